"""GPU: temporal attention over frame counts that do not divide 32 (attention_temporal_any.hip, ALPRO_ATTN_MAX_T) -- the windowed forward and the
one-launch backward behind alpro_attn_temporal_fwd / alpro_attn_temporal_bwd -- against torch fp64 on identical (pre-rounded) operands, with
the tolerances of the block-diagonal kernels.  T dividing 32 keeps those kernels: recorded hashes pin T = 8 and T = 16."""
import hashlib

import pytest
import torch

from tests.test_hip_bwd_ops import GRAD_TOL
from tests.test_hip_ops import DTYPES, FWD_TOL, _hip, attn_inputs, close, logit_atol, logit_rel_err, ref_attention, rnd, temporal_lse_rows

pytestmark = pytest.mark.gpu

H = 12
MAX_T = 128   # ALPRO_ATTN_MAX_T

# (T, groups): T below and above 32, group counts of 1, row counts that leave a ragged last 32-row chunk (rows % 32 != 0), the bound
FWD_CASES = [(3, 1), (3, 45), (5, 13), (6, 37), (7, 9), (12, 1), (12, 27), (17, 5), (24, 11), (31, 3), (33, 1), (33, 4), (48, 5), (64, 3),
             (96, 2), (127, 3), (128, 1), (128, 3)]
BWD_CASES = [(3, 45), (6, 37), (12, 27), (17, 5), (31, 3), (33, 4), (48, 5), (96, 2), (127, 2), (128, 1), (128, 3)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("T,groups", FWD_CASES)
def test_temporal_any_fwd(dt, T, groups):
    hip = _hip()
    rows = groups * T
    qkv = rnd(rows, 3 * H * 64, seed=1100 + T + groups).to(dt)
    out, lse = hip.attn_temporal(qkv.cuda(), T, H, 0.125, want_lse=True)
    ref, ref_lse = ref_attention(qkv.double(), groups, T, H, 0.125)
    close(out, ref, *FWD_TOL[dt], "temporal T=%d out" % T)
    assert lse.shape == ((rows + 31) // 32, H, 32)
    close(temporal_lse_rows(lse, rows, H), ref_lse.permute(0, 2, 1).reshape(rows, H), 1e-5, 1e-4, "temporal T=%d lse" % T)
    assert torch.equal(hip.attn_temporal(qkv.cuda(), T, H, 0.125), out)   # without lse: the same kernel, the same output


def _check_bwd(dt, qkv, dout, T, groups):
    """alpro_attn_temporal_fwd + _bwd against fp64 autograd.  As in test_hip_bwd_ops.check_attn_bwd, atol scales with max(1, max|ref|) and the
    reference takes delta = rowsum(dO o O) from the stored output (the backward's contract); fp32 adds the logit rounding bound."""
    hip = _hip()
    rows = groups * T
    out, lse = hip.attn_temporal(qkv.cuda(), T, H, 0.125, want_lse=True)
    dqkv = hip.attn_temporal_bwd(qkv.cuda(), out, dout.cuda(), lse, T, H, 0.125)
    q64 = qkv.double().requires_grad_(True)
    t = q64.view(groups, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    sm = ((t[0] @ t[1].transpose(-1, -2)) * 0.125).softmax(-1)
    o64 = sm @ t[2]
    do64 = dout.double().view(groups, T, H, 64).transpose(1, 2)
    o64.transpose(1, 2).reshape(rows, H * 64).backward(dout.double())
    g = q64.grad.view(rows, 3, H * 64).clone()
    extra = [0.0] * 3
    with torch.no_grad():
        t64 = qkv.double().view(groups, T, 3, H, 64).permute(2, 0, 3, 1, 4)
        dds = sm * (do64 * (out.cpu().double().view(groups, T, H, 64).transpose(1, 2) - o64)).sum(-1, keepdim=True)
        g[:, 0] -= (0.125 * dds @ t64[1]).transpose(1, 2).reshape(rows, H * 64)
        g[:, 1] -= (0.125 * dds.transpose(-1, -2) @ t64[0]).transpose(1, 2).reshape(rows, H * 64)
        rel = logit_rel_err(dt, qkv, None, groups, T, H)
        if rel:
            a, ado = t64.abs(), do64.abs()
            adp = ado @ a[2].transpose(-1, -2)
            ads = sm * (adp + (sm * adp).sum(-1, keepdim=True))
            extra = [2 * rel * float(x.abs().max()) for x in (0.125 * ads @ a[1], 0.125 * ads.transpose(-1, -2) @ a[0], sm.transpose(-1, -2) @ ado)]
    d = dqkv.view(rows, 3, H * 64)
    rtol, atol = GRAD_TOL[dt]
    for i, name in enumerate("QKV"):
        ref = g[:, i]
        close(d[:, i], ref, rtol, atol * max(1.0, float(ref.abs().max())) + extra[i], "d%s %s T=%d groups=%d" % (name, dt, T, groups))
    return out, lse, dqkv


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("T,groups", BWD_CASES)
def test_temporal_any_bwd(dt, T, groups):
    rows = groups * T
    qkv = (rnd(rows, 3 * H * 64, seed=1200 + T + groups) * 0.7).to(dt)
    dout = rnd(rows, H * 64, seed=1201 + T + groups).to(dt)
    _check_bwd(dt, qkv, dout, T, groups)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("regime", ["peaked", "late_max", "early_max", "offset"])
@pytest.mark.parametrize("T,groups", [(12, 27), (96, 2)])
def test_temporal_any_stress(dt, regime, T, groups):
    """attn_inputs with batch = groups and L = T is exactly the temporal layout: late_max plants the dominant key at each group's LAST frame
    (in a later 32-row tile than most of the group's queries), early_max at its first."""
    hip = _hip()
    qkv, _ = attn_inputs(groups, T, H, regime, "none", seed=T + 31 * groups)
    qkv = qkv.to(dt)
    out, lse = hip.attn_temporal(qkv.cuda(), T, H, 0.125, want_lse=True)
    ref, ref_lse = ref_attention(qkv.double(), groups, T, H, 0.125)
    rtol, atol = FWD_TOL[dt]
    close(out, ref, rtol, atol + logit_atol(dt, qkv, None, groups, T, H), "temporal %s T=%d out" % (regime, T))
    close(temporal_lse_rows(lse, groups * T, H), ref_lse.permute(0, 2, 1).reshape(-1, H), 1e-5, 1e-4, "temporal %s T=%d lse" % (regime, T))
    dout = rnd(groups * T, H * 64, seed=T + 7).to(dt)
    _check_bwd(dt, qkv, dout, T, groups)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("T,groups", [(12, 27), (48, 5)])
def test_temporal_any_deterministic(dt, T, groups):
    hip = _hip()
    rows = groups * T
    qkv = (rnd(rows, 3 * H * 64, seed=1300 + T) * 0.7).to(dt).cuda()
    dout = rnd(rows, H * 64, seed=1301 + T).to(dt).cuda()
    res = []
    for _ in range(2):
        out, lse = hip.attn_temporal(qkv, T, H, 0.125, want_lse=True)
        dqkv = hip.attn_temporal_bwd(qkv, out, dout, lse, T, H, 0.125)
        res.append((out, temporal_lse_rows(lse, rows, H), dqkv))
    for a, b in zip(*res):
        assert torch.equal(a.cpu(), b.cpu())


# Hashes recorded on the commit before the windowed kernels existed (T = 8 / 16 on the block-diagonal kernels, 37 / 19 groups: a ragged last
# chunk each): the seam leaves those T bit for bit.
SEAM_SHA256 = {
    "T16_bf16_dqkv": "b35976d2965e0d8e005119f5097a2419b19052e2b5fd26b6a2988c4bafe19826",
    "T16_bf16_lse": "4ac5707d232220499022fd707bbe82ff845483b1158e5cbe06527921b00c199d",
    "T16_bf16_out": "6446c36c2b087aa5e2a9f4e5a6262168973e9482731e4613ed2243de07692743",
    "T16_f16_dqkv": "a99a31c98fe17c49592dafcb8ca7310375efc94c5fac2856337c666b4a1c16c0",
    "T16_f16_lse": "652e3e3463eb8326e30888b5da6db380ecd514c8cbf5a101875bc60c49dd355a",
    "T16_f16_out": "4e5b67025f05ca158eec106d338f2651bef27625b68e3f238fee230ba0fe9a41",
    "T16_f32_dqkv": "092630836c539cf0079bb3d30e90968cc1acd1317216c05521037cbedb993138",
    "T16_f32_lse": "4d075acc9791d925563290e6774f761bb9aed8c09a908e43e23a62b937014d4e",
    "T16_f32_out": "55931c231075b252946f836cbba2acc69056e8f3290abb87e6c864aa46b8cc03",
    "T8_bf16_dqkv": "0f10316a7b4170179ca189fa75dc54f53fef0ea39c8ad80cbb9cfb8fa2270be1",
    "T8_bf16_lse": "623ffaef94ef2106219f2313b376d744f02ef626ede545b77cc6d5f257cd9f22",
    "T8_bf16_out": "93b03bcc681358ad98151a42c2a41e434d5f3cd75bd078ed5db2fc089b2009a2",
    "T8_f16_dqkv": "22ed519988feb120b3fc65f473eb8d03318278d24d3bd458672b1d847be5cdec",
    "T8_f16_lse": "01874b7a10b5c40ee81f2da7a2d6a6f60ee490eb79270068f0c62f1aeec8c651",
    "T8_f16_out": "68a1f9a5336cb83d7f8c52a5b36527d1307057ba1944db3b1a8ef75df4ce8482",
    "T8_f32_dqkv": "ce77e7d8122bd12e630c76a0d28dbc2019684a8a259de4c686ab10bcd41659d3",
    "T8_f32_lse": "6dcbccd2197ceae59e60d59707a0b3a336df15b0dad2f14ee351a91ab12f6658",
    "T8_f32_out": "538906aa0c65779e6294a8dfc0c810ec9ddf5059f52b772f18cbacd20b9fff29",
}


def _seam_outputs():
    hip = _hip()
    res = {}
    for T, groups in ((8, 37), (16, 19)):
        rows = T * groups
        for dt, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16"), (torch.float16, "f16")):
            qkv = (rnd(rows, 3 * H * 64, seed=970 + T) * 0.7).to(dt).cuda()
            dout = rnd(rows, H * 64, seed=971 + T).to(dt).cuda()
            out, lse = hip.attn_temporal(qkv, T, H, 0.125, want_lse=True)
            dqkv = hip.attn_temporal_bwd(qkv, out, dout, lse, T, H, 0.125)
            k = "T%d_%s" % (T, name)
            res[k + "_out"], res[k + "_lse"], res[k + "_dqkv"] = out, temporal_lse_rows(lse, rows, H), dqkv
    return {k: hashlib.sha256(v.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest() for k, v in res.items()}


def test_temporal_divisors_unchanged_bitwise():
    got = _seam_outputs()
    assert set(got) == set(SEAM_SHA256)
    for k, v in got.items():
        assert v == SEAM_SHA256[k], k


@pytest.mark.parametrize("T", [MAX_T + 1, 0])
def test_temporal_refuses_outside_bound(T):
    """The argument check fails before anything is launched: the error names ALPRO_ATTN_MAX_T's value."""
    hip = _hip()
    rows = max(T, 1) * 2
    qkv = torch.zeros(rows, 3 * H * 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="128"):
        hip.attn_temporal(qkv, T, H, 0.125, want_lse=True)
    out = torch.zeros(rows, H * 64, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros((rows + 31) // 32, H, 32, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="128"):
        hip.attn_temporal_bwd(qkv, out, out, lse, T, H, 0.125)


if __name__ == "__main__":   # prints the hashes SEAM_SHA256 records
    for k, v in sorted(_seam_outputs().items()):
        print('    "%s": "%s",' % (k, v))
