"""GPU: the block-diagonal temporal attention (T dividing 32: attn_temporal_fwd / attn_temporal_fwd16, the grouped attn_bwd<T, 1, 1, true> /
attn_temporal_bwd16, their _drop twins, alpro_gemm_qkv_tattn and the unit form of alpro_attn_temporal_probs) on the stress inputs of
tests/temporal_cases.py -- a cold group beside a hot one inside one 32-row unit, peaked / late_max / early_max / offset scores, ragged last
units, more units than one trip of the grid-stride loops covers -- against torch fp64 on the CPU on identical operands (the inputs are exact in
all three dtypes), every row compared.

Allowances: FWD_TOL (+ logit_atol, fp32) for outputs, (1e-5, 1e-4) for lse, and for gradients the scheme of test_hip_temporal_any._check_bwd --
GRAD_TOL with atol x max(1, max|ref|) per tensor, fp32 plus the logit rounding bound, and the reference's delta = rowsum(dO o O) taken from the
STORED output only where the kernel reads it (fp32; the 16-bit block-diagonal backward forms delta from P and dP).  Under dropout the absolute
parts carry 1 / (1 - p) as in test_hip_temporal_dropout.  tests/test_temporal_cases_cpu.py shows on the CPU that the kernels' own roundings stay
well inside these allowances on every case here and that a missing mask, a tile-wide row maximum, a stale K tile or a wrong lse row does not.
Every check prints its worst error / allowance ("RATIO|family|...") before it asserts."""
import functools

import pytest
import torch

from tests import attn_probs_cases as ac
from tests import attn_temporal_probs_cases as tpc
from tests import temporal_cases as tc
from tests.test_hip_bwd_ops import GRAD_TOL, _keep_mask
from tests.test_hip_ops import DTYPES, FWD_TOL, _hip, _on_grid, close, logit_atol, logit_rel_err, ref_attention, temporal_lse_rows

pytestmark = pytest.mark.gpu

SCALE = tc.SCALE
H = 12
P = 0.1
BITS16 = [torch.bfloat16, torch.float16]
DROP_CASES = [(2, 19), (8, 13), (16, 5), (32, 3)]
FUSED_CASES = [(1, 96), (2, 48), (4, 24), (8, 12), (16, 6)]   # 96 rows each: whole 32-row wave blocks, as the fused launch wants them
FUSED_H = 4                                                   # K = 768 = 3 * 4 * 64: the identity as weight


def _note(family, ratio, what):
    print("RATIO|%s|%.4f|%s" % (family, ratio, what))


@functools.lru_cache(maxsize=None)
def _case(kind, T, groups, heads=H, p=0.0):
    """Inputs and the fp64 reference of one case, computed once and shared by the dtypes and tests (never modified)."""
    qkv, dout = tc.inputs(kind, T, groups, heads, tc.seed_of(kind, T, groups, heads))
    seed, keep = 0, None
    if p:
        seed = (0x7E3D0000 + 977 * T + 31 * groups + int(p * 100)) | 1
        keep = _keep_mask(seed, groups * heads * T * T, p).view(groups, heads, T, T).double() / (1.0 - p)
    return dict(tc.reference(qkv, dout, T, heads, keep), qkv=qkv, dout=dout, keep=keep, seed=seed, T=T, groups=groups, H=heads, p=p,
                what="%s T=%d groups=%d H=%d p=%g" % (kind, T, groups, heads, p))


def _forward(c, dt, want_lse=True):
    return _hip().attn_temporal(c["qkv"].to(dt).cuda(), c["T"], c["H"], SCALE, want_lse=want_lse, drop_p=c["p"], drop_seed=c["seed"])


def _backward(c, dt, out, lse):
    return _hip().attn_temporal_bwd(c["qkv"].to(dt).cuda(), out, c["dout"].to(dt).cuda(), lse, c["T"], c["H"], SCALE, drop_p=c["p"], drop_seed=c["seed"])


def _check_fwd(c, dt, out, lse, family=None):
    T, groups, heads, mult = c["T"], c["groups"], c["H"], 1.0 / (1.0 - c["p"])
    family = family or ("fp32 forward" if dt == torch.float32 else "fwd16") + (" drop" if c["p"] else "")
    what = "%s %s" % (dt, c["what"])
    rtol, atol = FWD_TOL[dt]
    atol = (atol + logit_atol(dt, c["qkv"], None, groups, T, heads)) * mult
    lse_rows = temporal_lse_rows(lse, T * groups, heads)
    _note(family, tc.excess(out, c["out"], rtol, atol), "out " + what)
    _note(family, tc.excess(lse_rows, c["lse"], 1e-5, 1e-4), "lse " + what)
    assert lse.shape == ((T * groups + 31) // 32, heads, 32)
    close(out, c["out"], rtol, atol, "out " + what)
    close(lse_rows, c["lse"], 1e-5, 1e-4, "lse " + what)


def _check_bwd(c, dt, out, dqkv, family=None):
    """test_hip_temporal_any._check_bwd's scheme on a cached reference; with test_temporal_dropout_bwd's mask terms under dropout."""
    T, groups, heads, mult = c["T"], c["groups"], c["H"], 1.0 / (1.0 - c["p"])
    rows = T * groups
    family = family or ("grouped fp32 backward" if dt == torch.float32 else "bwd16") + (" drop" if c["p"] else "")
    what = "%s %s" % (dt, c["what"])
    qkv, sm, keep = c["qkv"], c["sm"], c["keep"]
    g = c["grad"]
    extra = [0.0] * 3
    if dt == torch.float32:   # the one dtype whose block-diagonal backward reads the stored output, and the one with a logit rounding bound
        t64 = qkv.double().view(groups, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
        do64 = c["dout"].double().view(groups, T, heads, 64).transpose(1, 2)
        g = g.clone()
        dds = sm * (do64 * (out.cpu().double().view(groups, T, heads, 64).transpose(1, 2) - c["o64"])).sum(-1, keepdim=True)
        g[:, 0] -= (SCALE * dds @ t64[1]).transpose(1, 2).reshape(rows, heads * 64)
        g[:, 1] -= (SCALE * dds.transpose(-1, -2) @ t64[0]).transpose(1, 2).reshape(rows, heads * 64)
        rel = logit_rel_err(dt, qkv, None, groups, T, heads)
        a, ado = t64.abs(), do64.abs()
        adp = ado @ a[2].transpose(-1, -2)
        pk = sm
        if keep is not None:
            adp, pk = adp * keep, sm * keep
        ads = sm * (adp + (sm * adp).sum(-1, keepdim=True))
        extra = [2 * rel * float(x.abs().max()) for x in (SCALE * ads @ a[1], SCALE * ads.transpose(-1, -2) @ a[0], pk.transpose(-1, -2) @ ado)]
    rtol, atol = GRAD_TOL[dt]
    for name, r in zip("QKV", tc.grad_excess(dqkv, g, rtol, atol, extra, mult)):
        _note(family, r, "d%s %s" % (name, what))
    d = dqkv.view(rows, 3, heads * 64)
    for i, name in enumerate("QKV"):
        ref = g[:, i]
        close(d[:, i], ref, rtol, atol * mult * max(1.0, float(ref.abs().max())) + extra[i], "d%s %s" % (name, what))


# ------------------------------------------------------------------------------------------------ 1. forward, lse and backward
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("T,groups", tc.DIAG_CASES)
def test_temporal_stress_fwd(dt, kind, T, groups):
    c = _case(kind, T, groups)
    out, lse = _forward(c, dt)
    _check_fwd(c, dt, out, lse)
    assert torch.equal(_forward(c, dt, want_lse=False), out)   # without lse: the same output bit for bit


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("T,groups", tc.DIAG_CASES)
def test_temporal_stress_bwd(dt, kind, T, groups):
    c = _case(kind, T, groups)
    out, lse = _forward(c, dt)
    _check_bwd(c, dt, out, _backward(c, dt, out, lse))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("heads", [1, 5])
def test_temporal_stress_mixed_groups_one_and_five_heads(dt, heads):
    """unit = chunk * H + head with H = 1 (every unit its own chunk) and H = 5 (units per workgroup of 4 waves straddle chunks)."""
    c = _case("mixed", 8, 13, heads)
    out, lse = _forward(c, dt)
    _check_fwd(c, dt, out, lse)
    assert torch.equal(_forward(c, dt, want_lse=False), out)
    _check_bwd(c, dt, out, _backward(c, dt, out, lse))


# ------------------------------------------------------------------------------------------------ 2. the dropout twins
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["mixed", "late_max"])
@pytest.mark.parametrize("T,groups", DROP_CASES)
def test_temporal_stress_dropout_fwd(dt, kind, T, groups):
    c = _case(kind, T, groups, H, P)
    out, lse = _forward(c, dt)
    _check_fwd(c, dt, out, lse)   # lse: that of the un-dropped row
    assert torch.equal(_forward(c, dt, want_lse=False), out)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["mixed", "late_max"])
@pytest.mark.parametrize("T,groups", DROP_CASES)
def test_temporal_stress_dropout_bwd(dt, kind, T, groups):
    c = _case(kind, T, groups, H, P)
    out, lse = _forward(c, dt)
    _check_bwd(c, dt, out, _backward(c, dt, out, lse))


# ------------------------------------------------------------------------------------------------ 3. the second trip of the grid-stride loops
@pytest.mark.parametrize("dt,p", [(torch.bfloat16, 0.0), (torch.float16, 0.0), (torch.bfloat16, P)])
def test_temporal_stress_more_units_than_one_trip_16_bit(dt, p):
    """2100 units on a grid capped at 512 x 4 waves: 52 waves take a second unit and reuse their LDS tiles.  Forward with lse and backward, every
    row against fp64; without dropout a second run gives the same bits."""
    T, groups = tc.MANY_UNITS_16
    c = _case("mixed", T, groups, tc.MANY_H, p)
    assert tc.units(T * groups, tc.MANY_H) > 2048
    out, lse = _forward(c, dt)
    dqkv = _backward(c, dt, out, lse)
    _check_fwd(c, dt, out, lse)
    _check_bwd(c, dt, out, dqkv)
    if not p:
        out2, lse2 = _forward(c, dt)
        assert torch.equal(out2, out) and torch.equal(lse2, lse) and torch.equal(_backward(c, dt, out2, lse2), dqkv)


@functools.lru_cache(maxsize=None)
def _many_units_32():
    T, groups = tc.MANY_UNITS_32
    qkv, _ = tc.inputs("mixed", T, groups, tc.MANY_H, tc.seed_of("mixed", T, groups))
    out, lse = ref_attention(qkv.double(), groups, T, tc.MANY_H, SCALE)
    return dict(qkv=qkv, out=out, lse=lse.permute(0, 2, 1).reshape(T * groups, tc.MANY_H), T=T, groups=groups, H=tc.MANY_H, p=0.0, seed=0,
                what="mixed T=%d groups=%d H=%d" % (T, groups, tc.MANY_H))


def test_temporal_stress_more_units_than_one_trip_fp32_forward():
    """8208 units on a grid capped at 2048 x 4 waves, the last unit ragged.  (The fp32 backward launches one workgroup per unit: no stride loop.)"""
    c = _many_units_32()
    assert tc.units(c["T"] * c["groups"], c["H"]) > 8192
    out, lse = _forward(c, torch.float32)
    _check_fwd(c, torch.float32, out, lse)


# ------------------------------------------------------------------------------------------------ 4. the fused qkv + attention launch
@pytest.mark.parametrize("dt", BITS16)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("kind", ["mixed", "late_max", "offset"])
@pytest.mark.parametrize("T,groups", FUSED_CASES)
def test_temporal_stress_fused_qkv_launch(dt, with_bias, kind, T, groups):
    """alpro_gemm_qkv_tattn with the identity as weight: every a . w + b is one product plus one addend, exact in fp32, so the q | k | v it returns
    must be the fp64 value rounded once to dt; its output and lse against fp64 of those q | k | v (and within 4 ulp of alpro_attn_temporal_fwd on
    them); its training form (q | k | v + lse) through the temporal backward against fp64 autograd."""
    hip = _hip()
    heads, rows = FUSED_H, T * groups
    K = 3 * heads * 64
    qkv, dout = tc.inputs(kind, T, groups, heads, tc.seed_of(kind, T, groups, heads))
    w = torch.eye(K).to(dt)
    b = None
    if with_bias:   # on the 2^-5 grid, |b| <= 1
        b = _on_grid(0.5 * torch.randn(K, generator=torch.Generator().manual_seed(900 + T)), 2.0 ** -5, 1.0)
        assert float(b.abs().max()) <= 1.0 and float(b.abs().max()) > 0.5
    a = (qkv if b is None else qkv - b).to(dt)
    assert hip.qkv_tattn_ok(a.cuda(), T)
    out3, qkv3, lse3 = hip.gemm_qkv_tattn(a.cuda(), w.cuda(), None if b is None else b.cuda(), T, heads, SCALE, want_qkv=True)
    want = (a.double() @ w.double().T + (0.0 if b is None else b.double())).to(dt)
    assert torch.equal(qkv3.cpu(), want), "q | k | v: %d elements differ from the exact value rounded once" % int((qkv3.cpu() != want).sum())
    assert torch.equal(hip.gemm_qkv_tattn(a.cuda(), w.cuda(), None if b is None else b.cuda(), T, heads, SCALE), out3)
    q32 = qkv3.float().cpu()
    c = dict(tc.reference(q32, dout, T, heads), qkv=q32, dout=dout, keep=None, seed=0, T=T, groups=groups, H=heads, p=0.0,
             what="fused %s T=%d bias=%s" % (kind, T, with_bias))
    _check_fwd(c, dt, out3, lse3, "fused")
    two = hip.attn_temporal(qkv3, T, heads, SCALE)
    d = (out3.float() - two.float()).abs().max().item()
    ulp = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dt] * max(1.0, two.float().abs().max().item())
    _note("fused", d / (4 * ulp), "out vs alpro_attn_temporal_fwd (4 ulp) %s %s" % (dt, c["what"]))
    assert d <= 4 * ulp, "fused vs alpro_attn_temporal_fwd on the same q | k | v: %.3e (ulp %.1e)" % (d, ulp)
    dqkv = hip.attn_temporal_bwd(qkv3, out3, dout.to(dt).cuda(), lse3, T, heads, SCALE)
    _check_bwd(c, dt, out3, dqkv, "fused")


# ------------------------------------------------------------------------------------------------ 5. the probabilities
@pytest.mark.parametrize("dtype", ac.DTYPES)
@pytest.mark.parametrize("T,groups", [(2, 19), (8, 13), (16, 5)])
def test_temporal_stress_probabilities(T, groups, dtype):
    """alpro_attn_temporal_probs (unit form) on the mixed input, lse from alpro_attn_temporal_fwd, inside attn_probs_cases' derived bound."""
    hip = _hip()
    heads, dt = 2, ac.TORCH_DTYPE[dtype]
    qkv, _ = tc.inputs("mixed", T, groups, heads, tc.seed_of("mixed", T, groups, heads))
    dev = qkv.to(dt).cuda()
    _, lse = hip.attn_temporal(dev, T, heads, SCALE, want_lse=True)
    p = hip.attn_temporal_probs(dev, lse, T, heads, SCALE)
    case = tpc.case_from_qkv("mixed_T%d_G%d_%s" % (T, groups, dtype), qkv.numpy(), groups, T, heads, dtype, SCALE)
    assert p.shape == (groups, heads, T, T) and p.dtype == torch.float32 and p.is_contiguous()
    _, ratio = ac.check(case, p.cpu().numpy(), tpc.lse_from_chunks(lse.cpu().numpy(), groups, T))
    _note("probs", ratio, case.name)
