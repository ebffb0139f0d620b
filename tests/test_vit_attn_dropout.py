"""attn_drop_rate in the visual encoder (vit.py:79,94: nn.Dropout on the softmax probabilities of the temporal AND the spatial attention).

CPU: the config key constructs, changes no state-dict key, drop_rate is still refused, the two new C symbols are declared and exported.
GPU: one train-mode Block against an fp64 restatement of vit.py:136-213 in plain torch that takes the attention keep masks (rebuilt from the seeds
the block saved, with the numpy replica of the hash) and the block's drop-path scales; then the properties that tie the paths together."""
import os

import pytest
import torch

from tests.test_hip_bwd_ops import _keep_mask
from tests.test_hip_ops import rnd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, H = 768, 12
P = 0.1
TOL = {"fp32": 2e-4, "fp16": 8e-4}   # tests/test_model_parity.py, block11_droppath_T2_B4: |err| <= tol * max|ref|


def test_attn_drop_rate_constructs_and_drop_rate_is_refused():
    from alpro_amd import hip
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    from tests.test_host_cpu import VENC
    cfg = dict(VENC, num_frm=2)
    m0 = TimeSformer(dict(cfg, attn_drop_rate=0.0), input_format="RGB")
    m1 = TimeSformer(dict(cfg, attn_drop_rate=0.1), input_format="RGB")
    assert list(m1.state_dict().keys()) == list(m0.state_dict().keys())
    blk = m1.model.blocks[3]
    assert isinstance(blk.attn.attn_drop, torch.nn.Dropout) and blk.attn.attn_drop.p == 0.1 and blk.temporal_attn.attn_drop.p == 0.1
    assert m0.model.blocks[3].attn.attn_drop.p == 0.0
    with pytest.raises(AssertionError, match="drop_rate"):
        TimeSformer(dict(cfg, drop_rate=0.1), input_format="RGB")
    header = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    for name in ("alpro_attn_temporal_fwd_drop", "alpro_attn_temporal_bwd_drop"):
        assert name in hip.EXPORTS and ("int %s(" % name) in header, name
    assert "#define ALPRO_HIP_ABI_VERSION 22" in header and hip.ABI_VERSION == 22


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
def _block(attn_drop, seed=21):
    from alpro_amd.modeling.timesformer.vit import Block
    torch.manual_seed(seed)
    blk = Block(dim=D, num_heads=H, layer_num=0, mlp_ratio=4.0, qkv_bias=True, drop_path=0.1, attn_drop=attn_drop, attention_type='divided_space_time')
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.3)
    return blk.cuda().train()


def _fix_drop_path(blk, B, T, N):
    g = torch.Generator().manual_seed(5)
    masks = {n: ((torch.rand(n, generator=g) > 0.25).float() / 0.75).cuda() for n in (B * N, B * T)}
    masks[B] = torch.tensor([1 / 0.75, 0.0] + [1 / 0.75] * (B - 2)).cuda()
    blk._drop = lambda rows, device: masks[rows]
    return masks


def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-6) * w + b


def _attention(x, p, pre, keep, scale):
    """x (G, L, D) -> proj(softmax(q k^T scale) o keep @ v); keep (G, H, L, L) already carries 1 / (1 - p)."""
    G, L, _ = x.shape
    qkv = (x @ p[pre + ".qkv.weight"].t() + p[pre + ".qkv.bias"]).view(G, L, 3, H, D // H).permute(2, 0, 3, 1, 4)
    prob = ((qkv[0] @ qkv[1].transpose(-1, -2)) * scale).softmax(-1) * keep
    o = (prob @ qkv[2]).transpose(1, 2).reshape(G, L, D)
    return o @ p[pre + ".proj.weight"].t() + p[pre + ".proj.bias"]


def _block_fp64(p, x, B, T, N, keep_t, keep_s, drop_t, drop_s, drop_m, scale):
    """vit.py:136-213 (divided space-time) on tokens in (b, 1 + (n t)) order, restated with views instead of rearranges."""
    cls, body = x[:, :1], x[:, 1:]
    xt = body.reshape(B * N, T, D)
    a_t = _attention(_ln(xt, p["temporal_norm1.weight"], p["temporal_norm1.bias"]), p, "temporal_attn", keep_t, scale) * drop_t[:, None, None]
    body = body + a_t.reshape(B, N * T, D) @ p["temporal_fc.weight"].t() + p["temporal_fc.bias"]
    frames = body.reshape(B, N, T, D).transpose(1, 2).reshape(B * T, N, D)
    xs = torch.cat([cls.expand(B, T, D).reshape(B * T, 1, D), frames], 1)
    a_s = _attention(_ln(xs, p["norm1.weight"], p["norm1.bias"]), p, "attn", keep_s, scale) * drop_s[:, None, None]
    cls2 = cls + a_s[:, 0].reshape(B, T, D).mean(1, keepdim=True)
    body2 = body + a_s[:, 1:].reshape(B, T, N, D).transpose(1, 2).reshape(B, N * T, D)
    x2 = torch.cat([cls2, body2], 1)
    hdn = _ln(x2, p["norm2.weight"], p["norm2.bias"]) @ p["mlp.fc1.weight"].t() + p["mlp.fc1.bias"]
    hdn = 0.5 * hdn * (1.0 + torch.erf(hdn * 0.7071067811865476))
    return x2 + (hdn @ p["mlp.fc2.weight"].t() + p["mlp.fc2.bias"]) * drop_m[:, None, None]


def _run(blk, x, dout, B, T, W, mode, seed=4242):
    from alpro_amd import config as rt
    for p in blk.parameters():
        p.grad = None
    rt.seed_dropout(seed)
    with rt.use_compute_dtype(mode), torch.no_grad():
        out, sv = blk.forward_train(x.clone(), B, T, W)
        seeds = sv["attn_drop"]
        dx, _ = blk.backward(sv, dout.clone())
    torch.cuda.synchronize()
    return out.clone(), dx.clone(), {n: p.grad.clone() for n, p in blk.named_parameters()}, seeds


@pytest.mark.gpu
@pytest.mark.parametrize("mode,T", [("fp32", 2), ("fp16", 2), ("fp32", 3)])
def test_block_attn_dropout_vs_fp64(mode, T):
    """B = 2, a 3 x 3 patch grid: 18 T temporal rows (T = 2: block-diagonal kernels, T = 3: windowed) and 2 T spatial sequences of L = 10."""
    B, W = 2, 3
    N = W * W
    S = 1 + N * T
    blk = _block(P)
    masks = _fix_drop_path(blk, B, T, N)
    x, dout = rnd(B, S, D, seed=600 + T), rnd(B, S, D, seed=601 + T)
    out, dx, grads, (p_t, seed_t, p_s, seed_s) = _run(blk, x.cuda(), dout.cuda(), B, T, W, mode)
    assert p_t == P and p_s == P and seed_t and seed_s and seed_t != seed_s
    keep_t = _keep_mask(seed_t, B * N * H * T * T, P).view(B * N, H, T, T).double() / (1.0 - P)
    keep_s = _keep_mask(seed_s, B * T * H * (N + 1) ** 2, P).view(B * T, H, N + 1, N + 1).double() / (1.0 - P)
    p64 = {n: p.detach().cpu().double().requires_grad_(True) for n, p in blk.named_parameters()}
    x64 = x.double().requires_grad_(True)
    ref = _block_fp64(p64, x64, B, T, N, keep_t, keep_s, masks[B * N].cpu().double(), masks[B * T].cpu().double(), masks[B].cpu().double(), blk.attn.scale)
    ref.backward(dout.double())
    tol = TOL[mode]
    worst = []
    for name, got, want in [("out", out, ref.detach()), ("dx", dx, x64.grad)] + [(n, grads[n], p64[n].grad) for n in sorted(p64)]:
        err, lim = float((got.cpu().double() - want).abs().max()), tol * float(want.abs().max())
        print("[attn-dropout block %s T=%d] %-28s err %.3e limit %.3e" % (mode, T, name, err, lim))
        if err > lim:
            worst.append((name, err, lim))
    assert not worst, worst


def _pair(B, T, W):
    """A block with attn_drop = 0.1, one with 0.0 and the same weights, the same fixed drop-path scales, inputs."""
    N = W * W
    S = 1 + N * T
    blk, blk0 = _block(P), _block(0.0)
    blk0.load_state_dict(blk.state_dict())
    _fix_drop_path(blk, B, T, N)
    _fix_drop_path(blk0, B, T, N)
    return blk, blk0, rnd(B, S, D, seed=610).cuda(), rnd(B, S, D, seed=611).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_block_attn_dropout_eval_and_p0_draw_nothing(mode):
    """Eval mode is the identity (bitwise the p = 0 model, no seed drawn); p = 0 draws no seed in train mode either."""
    from alpro_amd import config as rt
    B, T, W = 2, 2, 4
    blk, blk0, x, dout = _pair(B, T, W)
    blk.eval(), blk0.eval()
    rt.seed_dropout(7)
    with rt.use_compute_dtype(mode), torch.no_grad():
        assert torch.equal(blk(x.clone(), B, T, W), blk0(x.clone(), B, T, W))
    assert rt.dropout_state()[1] == 0
    blk0.train()
    _, _, _, seeds0 = _run(blk0, x, dout, B, T, W, mode)
    assert seeds0 == (0.0, 0, 0.0, 0) and rt.dropout_state()[1] == 0
    with rt.use_compute_dtype(mode), torch.no_grad():
        blk0(x.clone(), B, T, W)
    assert rt.dropout_state()[1] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_block_attn_dropout_train_mode_properties(mode):
    from alpro_amd import config as rt
    B, T, W = 2, 2, 4
    blk, blk0, x, dout = _pair(B, T, W)
    out0, _, _, _ = _run(blk0, x, dout, B, T, W, mode)
    # p > 0: two seeds per block and step, another output, and the same bits when the seed counter is reset
    out1, dx1, g1, seeds1 = _run(blk, x, dout, B, T, W, mode)
    assert rt.dropout_state()[1] == 2, rt.dropout_state()
    assert not torch.equal(out1, out0)
    out2, dx2, g2, seeds2 = _run(blk, x, dout, B, T, W, mode)
    assert seeds2 == seeds1
    assert torch.equal(out2, out1), "forward not reproducible"
    assert torch.equal(dx2, dx1), "input gradient not reproducible"
    diff = [n for n in g1 if not torch.equal(g1[n], g2[n])]
    assert not diff, diff
    # A train-mode forward under no_grad drops too, with the same seeds.  Block.forward is another kernel sequence than forward_train also at
    # p = 0 (in-place residual stream, deferred temporal add, the GELU without its saved derivative), so the two are compared at twice the
    # tolerance each keeps against the fp64 restatement; one wrong mask element moves an output by O(p) of an attention term, far above that.
    rt.seed_dropout(4242)
    with rt.use_compute_dtype(mode), torch.no_grad():
        y = blk(x.clone(), B, T, W)
    assert rt.dropout_state()[1] == 2, rt.dropout_state()
    err, lim = float((y - out1).abs().max()), 2 * TOL[mode] * float(out1.abs().max())
    print("[attn-dropout no_grad vs autograd path %s] err %.3e limit %.3e; p=0 vs p=0.1 differ by %.3e" % (mode, err, lim, float((out1 - out0).abs().max())))
    assert err <= lim, (err, lim)


@pytest.mark.gpu
def test_block_attn_dropout_skips_the_fused_temporal_launch():
    """alpro_gemm_qkv_tattn has no dropout: with ALPRO_FUSE_TATTN=1 and p > 0 every path that would take it runs the two launches instead, so
    the results are those of the unfused setting bit for bit (64 temporal rows: the fused launch would take them)."""
    from alpro_amd import config as rt
    from alpro_amd import hip
    B, T, W = 2, 2, 4
    N = W * W
    blk, _, x, dout = _pair(B, T, W)
    h = torch.empty((B * N * T, D), dtype=torch.float16, device="cuda")
    assert hip.qkv_tattn_ok(h, T)
    with rt.override("fuse_temporal_attention"):
        res = {}
        for fuse in ("0", "1"):
            rt.set_fuse_temporal_attention(fuse)
            res[fuse] = _run(blk, x, dout, B, T, W, "fp16")
            rt.seed_dropout(4242)
            with rt.use_compute_dtype("fp16"), torch.no_grad():
                res[fuse] += (blk(x.clone(), B, T, W),)
    assert torch.equal(res["1"][0], res["0"][0]) and torch.equal(res["1"][1], res["0"][1]) and torch.equal(res["1"][4], res["0"][4])
    assert all(torch.equal(res["1"][2][n], res["0"][2][n]) for n in res["0"][2])
