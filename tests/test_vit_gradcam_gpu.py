"""GPU: TimeSformer.forward_features(attn_grads=VitAttnGradients(...)) -- a collector changes no bit of `features`, of a gradient or of the
dropout-seed counter on every way a block can run its backward (plain with a clip gradient, with recomputation, behind a frozen prefix, with the
two temporal Linears unmerged, train mode with drop-path); with nothing trainable the pass is still anchored and ends at the first chosen block;
the refusals; every collected spatial and temporal G and CAM against an fp64 torch-autograd restatement of the encoder (retain_grad() on each
softmax); a spatial window; and grounding.frame_patch_gradcam / patch_temporal_gradcam on a small retrieval model.
img 48 (N = 9) x 2 frames (the unit form of the temporal kernel) and img 64 (N = 16) x 3 frames (the tile form), B = 2; closed-form weights; the
score is (features * pool_probe("temporal", shape)).sum().

Limits, as a fraction of a map's maximum: fp32 the project's exact-mode 2e-4, fp16 the 1e-2 that tests/test_model_parity.py applies to fp16
gradients against the reference -- the limits tests/test_gradcam_gpu.py uses for the same quantities of the text / fusion encoder."""
import math

import numpy as np
import pytest
import torch

from tests import test_model_parity as mp
from tests.conftest import BERT_CFG
from tests.golden.det_init import fill_state_dict_, unit_uniform
from tests.golden.make_golden_pool_modes import GEOMETRIES, pool_clips, pool_probe
from tests.test_host_cpu import VENC, make_cfg

pytestmark = pytest.mark.gpu

MODES = ["fp32", "fp16"]
TOL = {"fp32": 2e-4, "fp16": 1e-2}
SCALE = {"fp32": 1.0, "fp16": 4096.0}      # fp16 operands need a scaled backward: the scale of test_model_parity.backward
DEPTH, H, D = 12, 12, 768
GEO = {"img48": GEOMETRIES[1], "img64": GEOMETRIES[0]}
assert GEO["img48"] == dict(img=48, T=2, B=2) and GEO["img64"] == dict(img=64, T=3, B=2)


def _dims(name):
    g = GEO[name]
    return g["B"], g["T"], (g["img"] // 16) ** 2


@pytest.fixture(scope="module")
def cases():
    """name -> (encoder with drop-path 0.1 -- idle in eval mode -- and no attention dropout, clips (B, 3, T, img, img)), built once."""
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    built = {}

    def get(name):
        if name not in built:
            geo = GEO[name]
            enc = fill_state_dict_(TimeSformer(dict(VENC, num_frm=geo["T"], img_size=geo["img"], drop_path_rate=0.1), input_format="RGB"))
            built[name] = (enc.eval().cuda(), pool_clips(geo).cuda())
        enc, x = built[name]
        for p in enc.parameters():
            p.requires_grad_(True)
        return enc.eval(), x
    return get


def _collector(mode, **kw):
    from alpro_amd.modeling.timesformer.vit import VitAttnGradients
    return VitAttnGradients(grad_scale=SCALE[mode], **kw)


def _run(enc, x, mode, probe, col=None, x_grad=False, **flags):
    """One anchored forward + backward -> (features, {name: gradient}, clip gradient or None, dropout-seed counter behind it, the output object)."""
    from alpro_amd import config as rt
    mp.fresh_grads(enc)
    torch.manual_seed(1234)
    rt.seed_dropout(99)
    keep = mp.arm_scale(mode)
    xin = x.clone().requires_grad_(True) if x_grad else x
    kw = dict(flags, attn_grads=col) if col is not None else flags
    out = enc.forward_features(xin, **kw)
    feats = out if torch.is_tensor(out) else out.features
    assert feats.requires_grad
    mp.backward((feats * probe).sum(), mode)
    del keep
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
    return feats.detach().clone(), grads, (xin.grad.clone() if x_grad else None), list(rt.dropout_state()), out


def _check_shapes(col, B, T, N, layers=range(DEPTH)):
    for store, shape in ((col.spatial_grads, (B * T, H, 1 + N, 1 + N)), (col.spatial_cams, (B * T, H, 1 + N, 1 + N)),
                         (col.temporal_grads, (B * N, H, T, T)), (col.temporal_cams, (B * N, H, T, T))):
        assert sorted(store) == sorted(layers)
        for t in store.values():
            assert tuple(t.shape) == shape and t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad and bool(torch.isfinite(t).all())
    assert all(float(t.min()) >= 0 for t in list(col.spatial_cams.values()) + list(col.temporal_cams.values()))
    assert all(float(t.abs().max()) > 0 for t in list(col.spatial_grads.values()) + list(col.temporal_grads.values()))


VARIANTS = ["plain", "recompute", "frozen_prefix", "unmerged", "train_drop_path"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(GEO))
@pytest.mark.parametrize("mode", MODES)
def test_a_collector_changes_no_feature_gradient_or_seed(cases, monkeypatch, mode, name, variant):
    from alpro_amd import config as rt
    from alpro_amd.modeling.timesformer import vit
    enc, x = cases(name)
    B, T, N = _dims(name)
    probe = pool_probe("temporal", (B, 1 + N, D)).cuda()
    if variant == "unmerged":
        monkeypatch.setattr(vit.Block, "merge_temporal_proj", False)
    frozen = []
    if variant == "frozen_prefix":      # the embedding and the two leading blocks: they run the no-grad form (run_prefix_blocks)
        m = enc.model
        frozen = list(m.patch_embed.parameters()) + [m.cls_token, m.pos_embed, m.time_embed] + list(m.blocks[0].parameters()) + list(m.blocks[1].parameters())
    layers = range(2, DEPTH) if variant == "frozen_prefix" else range(DEPTH)     # (a chosen block inside the prefix would shorten it: the test below)
    x_grad = variant == "plain"        # the clip asks for a gradient in one variant
    if variant == "train_drop_path":
        enc.train()
    try:
        for p in frozen:
            p.requires_grad_(False)
        with rt.use_compute_dtype(mode), rt.use_recompute(variant == "recompute"):
            f0, g0, dx0, s0, _ = _run(enc, x, mode, probe, x_grad=x_grad)
            col = _collector(mode, layers=tuple(layers), want=("grad", "cam"))
            f1, g1, dx1, s1, _ = _run(enc, x, mode, probe, col=col, x_grad=x_grad)
    finally:
        enc.eval()
        for p in frozen:
            p.requires_grad_(True)
    assert torch.equal(f0, f1) and s0 == s1
    assert g0.keys() == g1.keys() and len(g0) > (100 if variant != "frozen_prefix" else 80)
    assert not [n for n in g0 if not torch.equal(g0[n], g1[n])]
    if x_grad:
        assert dx0 is not None and float(dx0.abs().max()) > 0 and torch.equal(dx0, dx1)
    if variant == "frozen_prefix":
        assert not [n for n in g0 if n.startswith(("model.blocks.0.", "model.blocks.1.", "model.patch_embed"))]
    _check_shapes(col, B, T, N, layers)


def test_recomputation_and_the_unmerged_projection_collect_the_plain_run_s_maps(cases, monkeypatch):
    """The replayed q | k | v and log-sum-exp rows are the first pass's bits, so the maps are; the unmerged projection hands the temporal half the
    same kind of d(ctx) (its bits may differ: two GEMMs instead of one), so its maps only need to be close."""
    from alpro_amd import config as rt
    from alpro_amd.modeling.timesformer import vit
    enc, x = cases("img64")
    B, T, N = _dims("img64")
    probe = pool_probe("temporal", (B, 1 + N, D)).cuda()
    cols = {}
    for variant in ("plain", "recompute", "unmerged"):
        with monkeypatch.context() as mctx, rt.use_compute_dtype("fp32"), rt.use_recompute(variant == "recompute"):
            if variant == "unmerged":
                mctx.setattr(vit.Block, "merge_temporal_proj", False)
            cols[variant] = _collector("fp32", layers=(0, 7, 11), want=("grad", "cam"))
            _run(enc, x, "fp32", probe, col=cols[variant])
    for i in (0, 7, 11):
        for what in ("spatial_grads", "spatial_cams", "temporal_grads", "temporal_cams"):
            a, b, c = (getattr(cols[v], what)[i] for v in ("plain", "recompute", "unmerged"))
            assert torch.equal(a, b), (what, i)
            assert float((a - c).abs().max()) <= TOL["fp32"] * float(a.abs().max()), (what, i)


def test_nothing_trainable_and_no_clip_gradient_the_backward_ends_at_the_first_chosen_block(cases, monkeypatch):
    from alpro_amd import config as rt
    from alpro_amd.modeling.timesformer import vit
    enc, x = cases("img64")
    B, T, N = _dims("img64")
    probe = pool_probe("temporal", (B, 1 + N, D)).cuda()
    with rt.use_compute_dtype("fp32"):
        ref = _collector("fp32", layers=(5, -1), want=("grad", "cam"))
        f_ref = _run(enc, x, "fp32", probe, col=ref)[0]                     # every parameter trainable
        calls = dict(train=[], backward=[], prefix=[])
        ft, bw, pf = vit.Block.forward_train, vit.Block.backward, vit.run_prefix_blocks
        monkeypatch.setattr(vit.Block, "forward_train", lambda self, *a, **k: (calls["train"].append(self.layer_num), ft(self, *a, **k))[1])
        monkeypatch.setattr(vit.Block, "backward", lambda self, *a, **k: (calls["backward"].append(self.layer_num), bw(self, *a, **k))[1])
        monkeypatch.setattr(vit, "run_prefix_blocks", lambda blocks, *a, **k: (calls["prefix"].append(len(blocks)), pf(blocks, *a, **k))[1])
        mp.fresh_grads(enc)
        for p in enc.parameters():
            p.requires_grad_(False)
        try:
            col = _collector("fp32", layers=(5, -1), want=("grad", "cam"))
            out = enc.forward_features(x, attn_grads=col)
            assert out.requires_grad                                        # anchored although nothing asks for a gradient
            with pytest.raises(RuntimeError, match=r"backward\(\) has not run"):
                col.spatial_cams
            (out * probe).sum().backward()
            torch.cuda.synchronize()
            assert all(p.grad is None for p in enc.parameters()) and x.grad is None
        finally:
            for p in enc.parameters():
                p.requires_grad_(True)
        with torch.no_grad():
            plain = enc.forward_features(x)
    assert calls["prefix"] == [5] and calls["train"] == list(range(5, DEPTH)) and calls["backward"] == list(range(DEPTH - 1, 4, -1))
    assert torch.equal(out.detach(), f_ref) and torch.equal(out.detach(), plain)
    _check_shapes(col, B, T, N, (5, 11))
    for what in ("spatial_grads", "spatial_cams", "temporal_grads", "temporal_cams"):     # frozen or not: the data gradient's bits
        assert all(torch.equal(getattr(col, what)[i], getattr(ref, what)[i]) for i in (5, 11)), what


def test_refusals(cases):
    from alpro_amd import config as rt
    enc, x = cases("img48")
    with rt.use_compute_dtype("fp32"):
        with torch.no_grad(), pytest.raises(RuntimeError, match="grad mode is off"):
            enc.forward_features(x, attn_grads=_collector("fp32"))
        with torch.no_grad(), pytest.raises(TypeError, match="forward_cls takes no attn_grads"):
            enc.forward_cls(x, attn_grads=_collector("fp32"))
        with pytest.raises(ValueError, match="block index -13 outside"):
            enc.forward_features(x, attn_grads=_collector("fp32", layers=(-13,)))
        blk = enc.model.blocks[4]
        enc.train()
        try:
            blk.temporal_attn.attn_drop.p = 0.1
            with pytest.raises(RuntimeError, match=r"block 4 has active attention dropout.*model\.eval\(\)"):
                enc.forward_features(x, attn_grads=_collector("fp32"))
            col = _collector("fp32", layers=(3, 5))                           # block 4 is not chosen: allowed, and drop-path stays allowed
            out = enc.forward_features(x, attn_grads=col)
            (out * out.detach()).sum().backward()
            assert sorted(col.spatial_cams) == [3, 5]
            enc.eval()                                                        # eval mode: the dropout is idle
            enc.forward_features(x, attn_grads=_collector("fp32"))
        finally:
            blk.temporal_attn.attn_drop.p = 0.0
            enc.eval()
            mp.fresh_grads(enc)


# ---- the fp64 autograd restatement of the encoder (vit.py:81-100, 146-212, 321-372, 484-492; eval mode) ------------------------------------------
def _ln64(x, ln):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), ln.weight.detach().double().cpu(), ln.bias.detach().double().cpu(), 1e-6)


def _lin64(x, lin):
    return x @ lin.weight.detach().double().cpu().t() + lin.bias.detach().double().cpu()


def _attn64(x, attn, probs):
    G, L, _ = x.shape
    qkv = _lin64(x, attn.qkv).view(G, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    p = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * attn.scale, dim=-1)
    p.retain_grad()
    probs.append(p)
    return _lin64((p @ qkv[2]).transpose(1, 2).reshape(G, L, D), attn.proj)


def restate64(enc, clips):
    """clips (B, 3, T, img, img) -> (features (B, 1 + N, D), spatial softmaxes, temporal softmaxes), fp64 on the CPU, each softmax with retain_grad()."""
    m = enc.model
    B, C, T, Hh, Ww = clips.shape
    N = (Hh // 16) * (Ww // 16)
    frames = clips.detach().double().cpu().requires_grad_(True).transpose(1, 2).reshape(B * T, C, Hh, Ww)   # (a leaf that asks: autograd records the graph)
    pe = m.patch_embed.proj
    rows = torch.nn.functional.conv2d(frames, pe.weight.detach().double().cpu(), pe.bias.detach().double().cpu(), stride=16).flatten(2).transpose(1, 2)   # (B*T, N, D)
    pos, time, cls = (t.detach().double().cpu() for t in (m.pos_embed, m.time_embed, m.cls_token))
    assert pos.shape[1] == 1 + N and time.shape[1] == T
    rows = rows + pos[:, 1:]
    rows = rows.view(B, T, N, D).transpose(1, 2) + time.view(1, 1, T, D)                        # (B, N, T, D)
    x = torch.cat([(cls + pos[:, :1]).expand(B, 1, D), rows.reshape(B, N * T, D)], 1)
    spatial, temporal = [], []
    for blk in m.blocks:
        xt = x[:, 1:].reshape(B * N, T, D)                                                      # 'b (n t) m -> (b n) t m'
        res_t = _lin64(_attn64(_ln64(xt, blk.temporal_norm1), blk.temporal_attn, temporal), blk.temporal_fc)
        xt = x[:, 1:] + res_t.reshape(B, N * T, D)
        cls_t = x[:, :1].repeat(1, T, 1).reshape(B * T, 1, D)
        xs = xt.reshape(B, N, T, D).transpose(1, 2).reshape(B * T, N, D)                        # 'b (n t) m -> (b t) n m'
        res_s = _attn64(_ln64(torch.cat([cls_t, xs], 1), blk.norm1), blk.attn, spatial)
        cls_res = res_s[:, 0].reshape(B, T, D).mean(1, keepdim=True)
        res = res_s[:, 1:].reshape(B, T, N, D).transpose(1, 2).reshape(B, N * T, D)
        x = torch.cat([x[:, :1], xt], 1) + torch.cat([cls_res, res], 1)
        u = _lin64(_ln64(x, blk.norm2), blk.mlp.fc1)
        x = x + _lin64(0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0))), blk.mlp.fc2)
    y = _ln64(x, m.norm)
    feats = torch.cat([y[:, :1], y[:, 1:].reshape(B, N, T, D).mean(2)], 1)
    return feats, spatial, temporal


@pytest.fixture(scope="module")
def restated(cases):
    """name -> (features64, [(P, G) spatial per block], [(P, G) temporal per block]) under the pool_probe score, computed once."""
    done = {}

    def get(name):
        if name not in done:
            enc, x = cases(name)
            with torch.enable_grad():
                feats, sp, tp = restate64(enc, x)
                (feats * pool_probe("temporal", feats.shape).double()).sum().backward()
            done[name] = (feats.detach(), [(p.detach(), p.grad) for p in sp], [(p.detach(), p.grad) for p in tp])
        return done[name]
    return get


@pytest.mark.parametrize("name", list(GEO))
@pytest.mark.parametrize("mode", MODES)
def test_every_collected_gradient_and_cam_against_the_fp64_restatement(cases, restated, mode, name):
    from alpro_amd import config as rt
    enc, x = cases(name)
    B, T, N = _dims(name)
    probe = pool_probe("temporal", (B, 1 + N, D)).cuda()
    feats64, sp64, tp64 = restated(name)
    col = _collector(mode, want=("grad", "cam"))
    with rt.use_compute_dtype(mode):
        feats, _, _, _, out = _run(enc, x, mode, probe, col=col, output_attentions=True, output_hidden_states=True)
    _check_shapes(col, B, T, N)
    assert float((feats.double().cpu() - feats64).abs().max()) <= (1e-3 if mode == "fp32" else 6e-3) * float(feats64.abs().max())
    assert len(out.hidden_states) == DEPTH + 1 and len(out.spatial_attentions) == DEPTH == len(out.temporal_attentions)
    worst = dict(spatial_G=0.0, spatial_CAM=0.0, temporal_G=0.0, temporal_CAM=0.0)
    fails = []
    for i in range(DEPTH):
        for half, (p64, g64), grad, cam, p in (("spatial", sp64[i], col.spatial_grads[i], col.spatial_cams[i], out.spatial_attentions[i]),
                                               ("temporal", tp64[i], col.temporal_grads[i], col.temporal_cams[i], out.temporal_attentions[i])):
            assert torch.equal(cam, p * grad.clamp(min=0)), (half, i)          # P is the `attentions` entry of the same pass, bit for bit
            cam64 = p64 * g64.clamp(min=0)
            for what, got, ref in (("G", grad, g64), ("CAM", cam, cam64)):
                err, top = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
                worst[half + "_" + what] = max(worst[half + "_" + what], err / top)
                if err > TOL[mode] * top:
                    fails.append((half, what, i, err, top))
    print("\n[vit gradcam vs fp64 %s %s] worst error as a fraction of the map's maximum (limit %.0e): %s"
          % (mode, name, TOL[mode], ", ".join("%s %.3e" % kv for kv in sorted(worst.items()))))
    assert not fails, fails


@pytest.mark.parametrize("mode", MODES)
def test_a_spatial_window_is_the_slice_of_the_full_map(cases, mode):
    from alpro_amd import config as rt
    enc, x = cases("img64")
    B, T, N = _dims("img64")
    probe = pool_probe("temporal", (B, 1 + N, D)).cuda()
    with rt.use_compute_dtype(mode):
        full = _collector(mode, layers=(0, 11), want=("grad", "cam"))
        _run(enc, x, mode, probe, col=full)
        for (q0, q1), (k0, k1) in (((0, 1), (1, 1 + N)), ((2, N), (3, N + 1))):
            win = _collector(mode, layers=(0, 11), want=("grad", "cam"), spatial_window=((q0, q1), (k0, k1)))
            _run(enc, x, mode, probe, col=win)
            for i in (0, 11):
                assert tuple(win.spatial_grads[i].shape) == (B * T, H, q1 - q0, k1 - k0)
                assert torch.equal(win.spatial_grads[i], full.spatial_grads[i][:, :, q0:q1, k0:k1])
                assert torch.equal(win.spatial_cams[i], full.spatial_cams[i][:, :, q0:q1, k0:k1])
                assert torch.equal(win.temporal_cams[i], full.temporal_cams[i])        # the temporal maps are always whole
        only = _collector(mode, layers=(11,), want="cam", spatial=False)
        _run(enc, x, mode, probe, col=only)
        assert torch.equal(only.temporal_cams[11], full.temporal_cams[11])
        with pytest.raises(RuntimeError, match="spatial=False"):
            only.spatial_cams


# ---- the grounding helpers on a small retrieval model ----------------------------------------------------------------------------------------------
LT = 10


@pytest.fixture(scope="module")
def retrieval():
    """AlproForVideoTextRetrieval with the 2 text + 2 fusion layer BERT of tests/test_gradcam_gpu.py and the img 48 x 2 frames encoder."""
    from alpro_amd.modeling.alpro_models import AlproForVideoTextRetrieval
    geo = GEO["img48"]
    cfg = make_cfg(dict(BERT_CFG, num_hidden_layers=4, fusion_layer=2, vocab_size=2048, attention_probs_dropout_prob=0.0))
    m = fill_state_dict_(AlproForVideoTextRetrieval(cfg, dict(VENC, num_frm=geo["T"], img_size=geo["img"], drop_path_rate=0.1)))
    m = m.eval().cuda()
    B = geo["B"]
    ids = torch.from_numpy((110 + np.floor((unit_uniform("vit_gradcam/ids", B * LT) + 1.0) * 0.5 * 1900)).astype(np.int64).reshape(B, LT))
    ids[:, 0] = 101
    mask = torch.ones(B, LT, dtype=torch.long)
    mask[1, LT - 3:] = 0
    ids[1, LT - 3:] = 0
    clips = pool_clips(geo).transpose(1, 2).contiguous()                     # (B, T, C, H, W), as the models take them
    return m, ids.cuda(), mask.cuda(), clips.cuda()


def _manual(m, ids, mask, clips, layers, scale, spatial):
    """What the helpers do, spelled out with the public pieces -> the head and layer mean of the collected cams."""
    from alpro_amd import config as rt
    from alpro_amd.modeling.alpro_models import _linear32
    from alpro_amd.modeling.timesformer.vit import VitAttnGradients
    B, T = clips.shape[:2]
    N = (clips.shape[3] // 16) * (clips.shape[4] // 16)
    col = VitAttnGradients(layers=layers, want=("cam",), spatial=spatial, temporal=not spatial, spatial_window=((0, 1), (1, 1 + N)) if spatial else None,
                           grad_scale=scale)
    flags = [(p, p.requires_grad) for p in m.parameters()]
    for p, _ in flags:
        p.requires_grad_(False)
    try:
        with torch.no_grad():
            te = m._text_embeds(ids, mask)
        video = m.visual_encoder.forward_features(clips.transpose(1, 2), return_all_tokens=True, attn_grads=col)
        att = torch.cat([mask, torch.ones(B, video.shape[1], dtype=mask.dtype, device="cuda")], dim=1)
        out = m._fusion(torch.cat([te, video.to(te.dtype)], dim=1), att)
        score = _linear32(out[:, 0, :], m.itm_head)[:, 1].sum() * scale
        with rt.loss_scaling(object()):
            score.backward()
    finally:
        for p, f in flags:
            p.requires_grad_(f)
    cams = col.spatial_cams if spatial else col.temporal_cams
    acc = None
    for i in layers:
        c = cams[i % DEPTH].mean(dim=1)
        acc = c if acc is None else acc + c
    return acc / float(len(layers))


@pytest.mark.parametrize("layers", ((-1,), (0, 5, 11)))
def test_helpers_are_the_mean_of_the_collected_cams_and_leave_the_model_untouched(retrieval, layers):
    from alpro_amd import config as rt
    from alpro_amd.grounding import frame_patch_gradcam, patch_temporal_gradcam
    m, ids, mask, clips = retrieval
    B, T = clips.shape[:2]
    g = clips.shape[3] // 16
    frozen = [m.itm_head.bias, m.visual_encoder.model.blocks[3].mlp.fc1.weight]        # a mix of flags to be restored
    for q in frozen:
        q.requires_grad_(False)
    marker = torch.full_like(m.visual_encoder.model.norm.bias, 7.0)
    m.visual_encoder.model.norm.bias.grad = marker.clone()         # a .grad an earlier step left: stays as it is; None stays None
    try:
        flags = [q.requires_grad for q in m.parameters()]
        grads = [q.grad for q in m.parameters()]
        maps = {}
        for mode in ("fp32", "fp16"):
            with rt.use_compute_dtype(mode):
                seeds = list(rt.dropout_state())
                fp = frame_patch_gradcam(m, ids, mask, clips, layers=layers)
                pt = patch_temporal_gradcam(m, ids, mask, clips, layers=layers)
                assert list(rt.dropout_state()) == seeds
                assert [q.requires_grad for q in m.parameters()] == flags
                assert all(a is b for a, b in zip(grads, [q.grad for q in m.parameters()]))
                assert torch.equal(m.visual_encoder.model.norm.bias.grad, marker)
                scale = 65536.0 if mode == "fp16" else 1.0              # the helpers' default: LossScaler's initial scale under fp16
                want_fp = _manual(m, ids, mask, clips, layers, scale, True)
                want_pt = _manual(m, ids, mask, clips, layers, scale, False)
            assert fp.shape == (B, T, g, g) and pt.shape == (B, g, g, T, T) and fp.dtype == pt.dtype == torch.float32
            assert torch.equal(fp, want_fp.view(B, T, g, g)) and torch.equal(pt, want_pt.view(B, g, g, T, T))
            assert float(fp.max()) > 0 and float(fp.min()) >= 0 and float(pt.max()) > 0 and float(pt.min()) >= 0
            maps[mode] = (fp, pt)
        for what, a, b in (("frame_patch_gradcam", maps["fp16"][0], maps["fp32"][0]), ("patch_temporal_gradcam", maps["fp16"][1], maps["fp32"][1])):
            err, top = float((a - b).abs().max()), float(b.max())
            print("[vit gradcam] %s layers=%s: fp16 (default grad_scale 2^16) vs fp32 max err %.3e = %.3e of max %.3e (limit %.0e)"
                  % (what, layers, err, err / top, top, TOL["fp16"]))
            assert err <= TOL["fp16"] * top
    finally:
        for q in frozen:
            q.requires_grad_(True)
        mp.fresh_grads(m)
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
        frame_patch_gradcam(m.train(), ids, mask, clips)
    m.eval()
    with pytest.raises(ValueError, match="layer 12 outside the 12 blocks"):
        patch_temporal_gradcam(m, ids, mask, clips, layers=(12,))
