"""GPU: dropout on the probabilities of the temporal attention (alpro_attn_temporal_fwd_drop / alpro_attn_temporal_bwd_drop; vit.py:79,94 on the
temporal half) -- the block-diagonal kernels (T | 32) and the windowed kernels (any other T) -- against torch fp64 on identical (pre-rounded)
operands with the mask restated in numpy, and against the spatial kernel, which draws the same mask for batch = groups, L = T.

Tolerances: FWD_TOL / GRAD_TOL of the temporal tests without dropout, the absolute part times 1 / (1 - p) (every kept probability, and with it
every output and every gradient term, carries that factor).  As in test_temporal_any_bwd the gradient's atol scales with max(1, max|ref|), fp32 adds
the logit rounding bound, and where the kernel takes delta = rowsum(dO o O) from the STORED output the reference does too."""
import pytest
import torch

from tests.test_hip_bwd_ops import GRAD_TOL, _keep_mask
from tests.test_hip_ops import DTYPES, FWD_TOL, _hip, close, logit_rel_err, rnd, temporal_lse_rows

pytestmark = pytest.mark.gpu

H = 3
SCALE = 0.125
PS = [0.1, 0.5]
# (T, groups); rows = T * groups is never a multiple of 32 (ragged last tile); the windowed cases cross tile boundaries mid-group
DIAG_CASES = [(1, 37), (2, 19), (8, 13), (16, 5), (32, 3)]
WINDOW_CASES = [(3, 11), (6, 27), (12, 27), (48, 5), (96, 2)]
CASES = DIAG_CASES + WINDOW_CASES
_CACHE = {}


def _seed(T, groups, p):
    return (0x5EED0000 + 977 * T + 31 * groups + int(p * 100)) | 1


def _case(T, groups, p, dt):
    """Inputs and the fp64 reference of one case, computed once and shared by the tests (never modified)."""
    key = (T, groups, p, dt)
    if key not in _CACHE:
        rows = T * groups
        qkv = (rnd(rows, 3 * H * 64, seed=2100 + T + groups) * 0.7).to(dt)
        dout = rnd(rows, H * 64, seed=2101 + T + groups).to(dt)
        seed = _seed(T, groups, p)
        keep = _keep_mask(seed, groups * H * T * T, p).view(groups, H, T, T).double() / (1.0 - p)
        q64 = qkv.double().requires_grad_(True)
        t = q64.view(groups, T, 3, H, 64).permute(2, 0, 3, 1, 4)
        s = (t[0] @ t[1].transpose(-1, -2)) * SCALE
        sm = s.softmax(-1)
        o64 = (sm * keep) @ t[2]
        ref = o64.transpose(1, 2).reshape(rows, H * 64)
        ref.backward(dout.double())
        _CACHE[key] = dict(qkv=qkv, dout=dout, seed=seed, keep=keep, ref=ref.detach(), lse=torch.logsumexp(s.detach(), -1).permute(0, 2, 1).reshape(rows, H),
                           grad=q64.grad.view(rows, 3, H * 64), sm=sm.detach(), o64=o64.detach())
    return _CACHE[key]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("T,groups", CASES)
def test_temporal_dropout_fwd(dt, p, T, groups):
    """softmax(q k^T scale) o keep / (1 - p) @ v with keep at index ((g H + h) T + q) T + k; lse is that of the un-dropped row."""
    hip = _hip()
    c = _case(T, groups, p, dt)
    rows = T * groups
    out, lse = hip.attn_temporal(c["qkv"].cuda(), T, H, SCALE, want_lse=True, drop_p=p, drop_seed=c["seed"])
    rtol, atol = FWD_TOL[dt]
    close(out, c["ref"], rtol, atol / (1.0 - p), "temporal dropout T=%d p=%g out" % (T, p))
    close(temporal_lse_rows(lse, rows, H), c["lse"], 1e-5, 1e-4, "temporal dropout T=%d lse" % T)
    assert torch.equal(hip.attn_temporal(c["qkv"].cuda(), T, H, SCALE, drop_p=p, drop_seed=c["seed"]), out)   # without lse: the same output


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("T,groups", CASES)
def test_temporal_dropout_fwd_equals_spatial_kernel(dt, p, T, groups):
    """alpro_attn_fwd with batch = groups, L = T has the same mask contract: the same elements are dropped."""
    hip = _hip()
    c = _case(T, groups, p, dt)
    out = hip.attn_temporal(c["qkv"].cuda(), T, H, SCALE, drop_p=p, drop_seed=c["seed"])
    spatial = hip.attn(c["qkv"].cuda(), groups, T, H, SCALE, drop_p=p, drop_seed=c["seed"])
    rtol, atol = FWD_TOL[dt]
    close(out, spatial.cpu().double(), 2 * rtol, 2 * atol / (1.0 - p), "temporal vs spatial dropout T=%d p=%g" % (T, p))   # two kernels, each within FWD_TOL of fp64


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("T,groups", CASES)
def test_temporal_dropout_bwd(dt, p, T, groups):
    """fp64 autograd through the masked expression.  The fp32 kernels and the windowed kernels read the stored output for delta (the 16-bit
    block-diagonal kernel forms delta from P and dP instead), so for them the reference's delta is taken from the stored output as well."""
    hip = _hip()
    c = _case(T, groups, p, dt)
    rows = T * groups
    qkv, dout, keep, sm = c["qkv"], c["dout"], c["keep"], c["sm"]
    out, lse = hip.attn_temporal(qkv.cuda(), T, H, SCALE, want_lse=True, drop_p=p, drop_seed=c["seed"])
    dqkv = hip.attn_temporal_bwd(qkv.cuda(), out, dout.cuda(), lse, T, H, SCALE, drop_p=p, drop_seed=c["seed"])
    g = c["grad"].clone()
    t64 = qkv.double().view(groups, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    do64 = dout.double().view(groups, T, H, 64).transpose(1, 2)
    reads_out = dt == torch.float32 or 32 % T != 0
    if reads_out:
        dds = sm * (do64 * (out.cpu().double().view(groups, T, H, 64).transpose(1, 2) - c["o64"])).sum(-1, keepdim=True)
        g[:, 0] -= (SCALE * dds @ t64[1]).transpose(1, 2).reshape(rows, H * 64)
        g[:, 1] -= (SCALE * dds.transpose(-1, -2) @ t64[0]).transpose(1, 2).reshape(rows, H * 64)
    extra = [0.0] * 3
    rel = logit_rel_err(dt, qkv, None, groups, T, H)
    if rel:   # fp32: the rounding of the logits, through |dS| and |P| (test_temporal_any_bwd's bound with the mask's scale on dP and P)
        a, ado = t64.abs(), do64.abs()
        adp = keep * (ado @ a[2].transpose(-1, -2))
        ads = sm * (adp + (sm * adp).sum(-1, keepdim=True))
        extra = [2 * rel * float(x.abs().max()) for x in (SCALE * ads @ a[1], SCALE * ads.transpose(-1, -2) @ a[0], (sm * keep).transpose(-1, -2) @ ado)]
    d = dqkv.view(rows, 3, H * 64)
    rtol, atol = GRAD_TOL[dt]
    for i, name in enumerate("QKV"):
        ref = g[:, i]
        close(d[:, i], ref, rtol, atol / (1.0 - p) * max(1.0, float(ref.abs().max())) + extra[i], "d%s %s T=%d groups=%d p=%g" % (name, dt, T, groups, p))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("T,groups", [(8, 13), (12, 27)])
def test_temporal_dropout_off_is_the_old_entry_point_bitwise(dt, T, groups):
    """drop_p == 0 (any seed) and drop_seed == 0 (any p) through the new entry points: the kernels of the old ones, forward and backward."""
    hip = _hip()
    c = _case(T, groups, 0.1, dt)
    qkv, dout = c["qkv"].cuda(), c["dout"].cuda()
    out0, lse0 = hip.attn_temporal(qkv, T, H, SCALE, want_lse=True)
    dqkv0 = hip.attn_temporal_bwd(qkv, out0, dout, lse0, T, H, SCALE)
    for kw in (dict(drop_p=0.0, drop_seed=12345), dict(drop_p=0.1, drop_seed=0)):
        out, lse = hip.attn_temporal(qkv, T, H, SCALE, want_lse=True, **kw)
        dqkv = hip.attn_temporal_bwd(qkv, out0, dout, lse0, T, H, SCALE, **kw)
        assert torch.equal(out, out0) and torch.equal(dqkv, dqkv0), kw
        assert torch.equal(temporal_lse_rows(lse, T * groups, H), temporal_lse_rows(lse0, T * groups, H)), kw


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("T,groups", [(8, 13), (12, 27), (48, 5)])
def test_temporal_dropout_deterministic(dt, T, groups):
    """No atomics, no workspace: one seed twice gives the same bits, forward and backward; another seed gives another mask."""
    hip = _hip()
    c = _case(T, groups, 0.1, dt)
    qkv, dout, seed = c["qkv"].cuda(), c["dout"].cuda(), c["seed"]
    res = []
    for _ in range(2):
        out, lse = hip.attn_temporal(qkv, T, H, SCALE, want_lse=True, drop_p=0.1, drop_seed=seed)
        res.append((out, temporal_lse_rows(lse, T * groups, H), hip.attn_temporal_bwd(qkv, out, dout, lse, T, H, SCALE, drop_p=0.1, drop_seed=seed)))
    for a, b in zip(*res):
        assert torch.equal(a.cpu(), b.cpu())
    other, lse = hip.attn_temporal(qkv, T, H, SCALE, want_lse=True, drop_p=0.1, drop_seed=seed + 2)
    assert not torch.equal(other, res[0][0])
    assert torch.equal(temporal_lse_rows(lse, T * groups, H), res[0][1])   # lse does not see the mask
    assert not torch.equal(hip.attn_temporal_bwd(qkv, other, dout, lse, T, H, SCALE, drop_p=0.1, drop_seed=seed + 2), res[0][2])


@pytest.mark.parametrize("T", [8, 12])
@pytest.mark.parametrize("p", [1.0, -0.1])
def test_temporal_dropout_refuses_p_outside_the_bound(T, p):
    """The argument check fails before anything is launched, and the message names the bound."""
    hip = _hip()
    rows = T * 4
    qkv = torch.zeros(rows, 3 * H * 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match=r"0 <= p < 1"):
        hip.attn_temporal(qkv, T, H, SCALE, want_lse=True, drop_p=p, drop_seed=7)
    out = torch.zeros(rows, H * 64, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros((rows + 31) // 32, H, 32, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match=r"0 <= p < 1"):
        hip.attn_temporal_bwd(qkv, out, out, lse, T, H, SCALE, drop_p=p, drop_seed=7)
