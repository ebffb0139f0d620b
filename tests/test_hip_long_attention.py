"""GPU: attention over L > 256 tokens (attention_long.hip, ABI 21) -- the key-blocked forward and the two-kernel backward behind
alpro_attn_fwd / alpro_attn_bwd -- against torch fp64 on identical (pre-rounded) operands, with the tolerances of the whole-row kernels."""
import hashlib

import pytest
import torch

from tests.test_hip_bwd_ops import GRAD_TOL, _keep_mask, attn_ref, check_attn_bwd
from tests.test_hip_ops import DTYPES, _hip, check_attn_fwd, close, ref_attention, rnd

pytestmark = pytest.mark.gpu

H = 12
MAX_L = 1024   # ALPRO_ATTN_MAX_L
FWD_TOL = {torch.float32: (2e-5, 2e-5), torch.bfloat16: (2e-2, 2e-2), torch.float16: (3e-3, 3e-3)}


def _bias(batch, L, seed):
    """(1 - mask) * -10000 with a different padded tail per sequence (the tails cross key-block boundaries)."""
    m = torch.ones(batch, L)
    for b in range(batch):
        m[b, L - 3 - (37 * b + seed) % (L // 3):] = 0
    return (1.0 - m) * -10000.0


FWD_CASES = [(2, 257, False), (2, 293, False), (2, 320, True), (1, 511, False), (1, 512, False), (2, 513, False), (2, 517, True),
             (1, 709, False), (1, 1024, False),
             # last key block of 1 / 32 / 33 / 63 / 64 keys; exact and ragged 128-query workgroups; the bound, masked, two sequences
             (2, 257, True), (2, 288, True), (2, 289, True), (1, 319, True), (1, 384, True), (2, 385, True), (2, 1023, True), (2, 1024, True)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("batch,L,masked", FWD_CASES)
def test_long_attn_fwd(dt, batch, L, masked):
    hip = _hip()
    qkv = rnd(batch * L, 3 * H * 64, seed=500 + L).to(dt)
    bias = _bias(batch, L, L) if masked else None
    out, lse = hip.attn(qkv.cuda(), batch, L, H, 0.125, None if bias is None else bias.cuda(), want_lse=True)
    ref, ref_lse = ref_attention(qkv.double(), batch, L, H, 0.125, bias)
    close(out, ref, *FWD_TOL[dt], "long attn out")
    close(lse, ref_lse, 1e-5, 1e-4, "long attn lse")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("batch,L,masked", [(2, 257, False), (2, 320, True), (1, 513, False), (2, 517, True), (1, 709, False),
                                            (2, 288, True), (2, 289, False), (1, 319, True), (2, 384, True), (1, 385, False), (1, 1023, True),
                                            (1, 1024, False)])
def test_long_attn_bwd(dt, batch, L, masked):
    hip = _hip()
    qkv = (rnd(batch * L, 3 * H * 64, seed=600 + L) * 0.7).to(dt)
    dout = rnd(batch * L, H * 64, seed=601 + L).to(dt)
    bias = _bias(batch, L, 7) if masked else None
    q64 = qkv.double().requires_grad_(True)
    attn_ref(q64, batch, L, H, 0.125, bias).backward(dout.double())
    kb = None if bias is None else bias.cuda()
    out, lse = hip.attn(qkv.cuda(), batch, L, H, 0.125, kb, want_lse=True)
    dqkv = hip.attn_bwd(qkv.cuda(), out, dout.cuda(), lse, batch, L, H, 0.125, kb)
    g = q64.grad.view(batch * L, 3, H * 64)
    d = dqkv.view(batch * L, 3, H * 64)
    for i, name in enumerate("QKV"):
        close(d[:, i], g[:, i], *GRAD_TOL[dt], "long d%s" % name)


# (batch, L, H, regime, mask) for the key-blocked path: the stress regimes x the fusion mask (a fully masked 64-key block between valid ones at
# L = 385 / 1024 for the sequences that keep 1 or 2 text keys) and the single mask; one head (grid 3 / 4 workgroups, no XCD remap) and 16 heads
# (grid 2 * 16 * 4 = 128, remapped); H = 12, batch 2: grids 72 / 96 / 192 (remapped)
ATTN_STRESS_LONG = ([(2, L, 12, r, m) for L in (289, 385, 1024) for r in ("peaked", "late_max", "offset") for m in ("fusion", "single")]
                    + [(4, 320, 12, "gauss", "fusion"), (2, 1023, 12, "early_max", "fusion"), (2, 257, 12, "late_max", "tail"), (2, 319, 12, "gauss", "all"),
                       (2, 319, 12, "offset", "all"), (2, 384, 12, "late_max", "none"), (1, 289, 1, "peaked", "fusion"), (2, 385, 16, "late_max", "fusion")])
ATTN_STRESS_BWD_LONG = ([(2, 385, 12, r, m) for r in ("peaked", "late_max", "offset") for m in ("fusion", "single")]
                        + [(2, 1023, 12, "late_max", "fusion"), (2, 1024, 12, "peaked", "single"), (2, 1024, 12, "offset", "fusion"),
                           (2, 319, 12, "gauss", "all"), (1, 385, 1, "peaked", "fusion"), (2, 289, 16, "late_max", "fusion")])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("batch,L,H,regime,mask", ATTN_STRESS_LONG)
def test_long_attn_stress_fwd(dt, batch, L, H, regime, mask):
    check_attn_fwd(dt, batch, L, H, regime, mask, seed=L + 7 * H)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("batch,L,H,regime,mask", ATTN_STRESS_BWD_LONG)
def test_long_attn_stress_bwd(dt, batch, L, H, regime, mask):
    check_attn_bwd(dt, batch, L, H, regime, mask, seed=5 * L + H)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("L,masked", [(293, False), (517, True)])
def test_long_attn_dropout_fwd_bwd(dt, L, masked):
    """Attention-probability dropout: the mask drop_keep(seed, ((b*H+h)*L+q)*L+key) of the whole-row kernels, restated in numpy; the softmax
    normaliser sums the un-dropped probabilities."""
    hip = _hip()
    batch, p, seed = 2, 0.1, 777
    qkv = (rnd(batch * L, 3 * H * 64, seed=700 + L) * 0.7).to(dt)
    dout = rnd(batch * L, H * 64, seed=701 + L).to(dt)
    bias = _bias(batch, L, 3) if masked else None
    keep = _keep_mask(seed, batch * H * L * L, p).view(batch, H, L, L).double()
    q64 = qkv.double().requires_grad_(True)
    t = q64.view(batch, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (t[0] @ t[1].transpose(-1, -2)) * 0.125
    if bias is not None:
        s = s + bias[:, None, None, :].double()
    ref = ((s.softmax(-1) * keep / (1 - p)) @ t[2]).transpose(1, 2).reshape(batch * L, H * 64)
    ref.backward(dout.double())
    kb = None if bias is None else bias.cuda()
    out, lse = hip.attn(qkv.cuda(), batch, L, H, 0.125, kb, want_lse=True, drop_p=p, drop_seed=seed)
    close(out, ref, *FWD_TOL[dt], "long attn dropout fwd")
    close(lse, torch.logsumexp(s, -1), 1e-5, 1e-4, "long attn dropout lse")
    dqkv = hip.attn_bwd(qkv.cuda(), out, dout.cuda(), lse, batch, L, H, 0.125, kb, drop_p=p, drop_seed=seed)
    close(dqkv, q64.grad, *GRAD_TOL[dt], "long attn dropout bwd")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("batch,L,group,masked,p", [(2, 320, 1, True, 0.0), (2, 320, 1, True, 0.1), (8, 325, 8, False, 0.0)])
def test_long_attn_cls_precise_query(dt, batch, L, group, masked, p):
    """The precise [CLS] query of alpro_attn_fwd at L > 256 (text form, cls_group 1; ViT form, one CLS row per clip of 8 frames): the fp32 q row
    against the 16-bit K / V of every key, key 0 included.  The k / v thirds of cls_q are NaN: they must never be read.  The regular output
    must not move."""
    hip = _hip()
    qkv = rnd(batch * L, 3 * H * 64, seed=800 + L).to(dt)
    cls = rnd(batch // group, 3 * H * 64, seed=801 + L)
    cls.view(batch // group, 3, H * 64)[:, 1:] = float("nan")
    bias = _bias(batch, L, 11) if masked else None
    seed = 4321 if p > 0 else 0
    kb = None if bias is None else bias.cuda()
    plain = hip.attn(qkv.cuda(), batch, L, H, 0.125, kb, drop_p=p, drop_seed=seed)
    full, fused = hip.attn(qkv.cuda(), batch, L, H, 0.125, kb, drop_p=p, drop_seed=seed, cls_q=cls.cuda(), cls_group=group)
    assert torch.equal(full, plain)
    t = qkv.double().view(batch, L, 3, H, 64)
    qc = cls.double().view(batch // group, 3, H, 64).repeat_interleave(group, 0)[:, 0]
    sc = torch.einsum("bhd,blhd->bhl", qc, t[:, :, 1]) * 0.125
    if bias is not None:
        sc = sc + bias[:, None, :].double()
    pr = sc.softmax(-1)
    if p > 0:   # the mask the forward draws for query 0 of (b, h)
        keep = _keep_mask(seed, batch * H * L * L, p).view(batch, H, L, L)[:, :, 0].double()
        pr = pr * keep / (1.0 - p)
    ref = torch.einsum("bhl,blhd->bhd", pr, t[:, :, 2]).reshape(batch, H * 64)
    assert torch.isfinite(fused).all()
    close(fused, ref, 2e-5, 2e-5, "long attn cls")


def test_long_attn_deterministic():
    """Two forward + backward runs at L = 517 (bf16, masked, dropout) are bitwise equal: no atomics anywhere."""
    hip = _hip()
    batch, L, p, seed = 3, 517, 0.1, 99
    qkv = (rnd(batch * L, 3 * H * 64, seed=900) * 0.7).to(torch.bfloat16).cuda()
    dout = rnd(batch * L, H * 64, seed=901).to(torch.bfloat16).cuda()
    kb = _bias(batch, L, 5).cuda()
    runs = []
    for _ in range(2):
        out, lse = hip.attn(qkv, batch, L, H, 0.125, kb, want_lse=True, drop_p=p, drop_seed=seed)
        dqkv = hip.attn_bwd(qkv, out, dout, lse, batch, L, H, 0.125, kb, drop_p=p, drop_seed=seed)
        runs.append((out, lse, dqkv))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# sha256 of the whole-row kernels' results at L = 256 on the inputs of _boundary_outputs, recorded from the build before the long-sequence
# path existed: L <= 256 keeps its kernels, bit for bit.
BOUNDARY_SHA256 = {
    "bf16_cls": "4c7e337a96a6107201a1e505de25657ab07df2278a15c10cc28a4f923dadcc23",
    "bf16_dqkv": "2e7eebf2691b14ded8cbae5805e7b657873c5db89e8bb1de58002c46834799ba",
    "bf16_lse": "fa32e52dff88aa73e40d8d4d425c04f05b71c2ea4484c9dcad5277fb54ebfdcc",
    "bf16_out": "74a0f1af3618f2b3ee9bd7029b12cc408cb1ffa938dd25c65753c86ba096284c",
    "f16_cls": "92fd9b975e40d6e433fb560fdbcd0587a19de2b6ec1e01fa88f3ba5fd6186178",
    "f16_dqkv": "541b382ab399a32b69bfcfe622f704ec2705ab6812077ee1c3a4127a93de9dbb",
    "f16_lse": "1bf1b6848ffd83aed54055ea5b5a6756c79414e4eb95c73004c8f1b14c3da22b",
    "f16_out": "fdb40a32f9aabef407f7fe4406cc594497cd87eb417bc67c75a40dffcba91d04",
    "f32_dqkv": "d5c4886044549c97d0961ce26e2b5059e72eeab415005d9a09bc3dbad9361a23",
    "f32_lse": "4f4376783940376f8e7a7771a441aa55ed028c9a29fd641ca0e3d908d6b8cc7c",
    "f32_out": "a7a06dd7629876859e7cdc2ed0e8ff4cae2d4eb318b2ae682d00f36d4100e38b",
}


def _boundary_outputs():
    hip = _hip()
    res = {}
    batch, L = 2, 256
    for dt, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16"), (torch.float16, "f16")):
        qkv = (rnd(batch * L, 3 * H * 64, seed=950) * 0.7).to(dt).cuda()
        dout = rnd(batch * L, H * 64, seed=951).to(dt).cuda()
        kb = _bias(batch, L, 1).cuda()
        out, lse = hip.attn(qkv, batch, L, H, 0.125, kb, want_lse=True, drop_p=0.1, drop_seed=31)
        dqkv = hip.attn_bwd(qkv, out, dout, lse, batch, L, H, 0.125, kb, drop_p=0.1, drop_seed=31)
        res[name + "_out"], res[name + "_lse"], res[name + "_dqkv"] = out, lse, dqkv
        if dt != torch.float32:
            cls = rnd(batch, 3 * H * 64, seed=952).cuda()
            res[name + "_cls"] = hip.attn(qkv, batch, L, H, 0.125, kb, cls_q=cls, cls_group=1)[1]
    return {k: hashlib.sha256(v.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest() for k, v in res.items()}


def test_l256_unchanged_bitwise():
    got = _boundary_outputs()
    assert set(got) == set(BOUNDARY_SHA256)
    for k, v in got.items():
        assert v == BOUNDARY_SHA256[k], k


def test_long_attn_refuses_above_bound():
    hip = _hip()
    L = MAX_L + 1
    qkv = torch.zeros(L, 3 * H * 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="1024"):
        hip.attn(qkv, 1, L, H, 0.125)
    out = torch.zeros(L, H * 64, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(1, H, L, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="1024"):
        hip.attn_bwd(qkv, out, out, lse, 1, L, H, 0.125)


if __name__ == "__main__":   # prints the hashes BOUNDARY_SHA256 records
    for k, v in sorted(_boundary_outputs().items()):
        print('    "%s": "%s",' % (k, v))
