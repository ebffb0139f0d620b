"""GPU: TimeSformer.forward_features(output_attentions=, output_hidden_states=, attn_layers=, attn_window=) -- shapes and selection, the bitwise
invariance of `features`, of every gradient and of the random streams on every way a block can run (no-grad eval, train mode, the anchored path,
with recomputation, behind a frozen prefix, with the two temporal Linears unmerged, one stream at B = 16), every map against an fp64 restatement of
its block computed from the returned hidden state, the CLS rows of the hidden states with the precise-CLS chain on and off its side stream, and the
two grounding helpers.  img 48 (N = 9) x 2 frames and img 64 (N = 16) x 3 frames (the windowed temporal path), B = 2; closed-form weights."""
import numpy as np
import pytest
import torch

from tests import test_model_parity as mp
from tests.golden.det_init import fill_state_dict_
from tests.golden.make_golden_pool_modes import GEOMETRIES, pool_clips, pool_probe
from tests.test_host_cpu import VENC

pytestmark = pytest.mark.gpu

MODES = ["fp32", "fp16"]
MAP_TOL = {"fp32": 2e-4, "fp16": 8e-4}
DEPTH, H, D = 12, 12, 768
GEO = {"img48": GEOMETRIES[1], "img64": GEOMETRIES[0]}
assert GEO["img48"] == dict(img=48, T=2, B=2) and GEO["img64"] == dict(img=64, T=3, B=2)


@pytest.fixture(scope="module")
def cases():
    """name -> (encoder with attention dropout 0.1 and drop-path 0.1 -- both idle in eval mode --, clips (B, 3, T, img, img)), built once."""
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    built = {}

    def get(name):
        if name not in built:
            geo = GEO[name]
            enc = fill_state_dict_(TimeSformer(dict(VENC, num_frm=geo["T"], img_size=geo["img"], drop_path_rate=0.1, attn_drop_rate=0.1), input_format="RGB"))
            built[name] = (enc.eval().cuda(), pool_clips(geo).cuda())
        enc, x = built[name]
        for p in enc.parameters():
            p.requires_grad_(True)
        return enc.eval(), x
    return get


@pytest.fixture(scope="module")
def full(cases):
    """(geometry, mode) -> the eval-mode output with both flags, computed once and left unchanged."""
    from alpro_amd import config as rt
    done = {}

    def get(name, mode):
        if (name, mode) not in done:
            enc, x = cases(name)
            with rt.use_compute_dtype(mode), torch.no_grad():
                done[(name, mode)] = enc.forward_features(x, output_attentions=True, output_hidden_states=True)
        return done[(name, mode)]
    return get


def _dims(name):
    g = GEO[name]
    return g["B"], g["T"], (g["img"] // 16) ** 2


@pytest.mark.parametrize("name", list(GEO))
@pytest.mark.parametrize("mode", MODES)
def test_shapes_counts_layers_and_window(cases, full, mode, name):
    from alpro_amd import config as rt
    from alpro_amd.modeling.timesformer.vit import VisualEncoderOutput
    enc, x = cases(name)
    B, T, N = _dims(name)
    out = full(name, mode)
    assert isinstance(out, VisualEncoderOutput) and tuple(out.features.shape) == (B, 1 + N, D)
    assert len(out.hidden_states) == DEPTH + 1 and len(out.spatial_attentions) == DEPTH and len(out.temporal_attentions) == DEPTH
    for t in out.hidden_states + out.spatial_attentions + out.temporal_attentions:
        assert t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad and bool(torch.isfinite(t).all())
    assert all(tuple(h.shape) == (B, 1 + N * T, D) for h in out.hidden_states)
    assert all(tuple(m.shape) == (B * T, H, 1 + N, 1 + N) for m in out.spatial_attentions)
    assert all(tuple(m.shape) == (B * N, H, T, T) for m in out.temporal_attentions)
    for m in out.spatial_attentions + out.temporal_attentions:    # fp32 sums of up to 17 probabilities, each within 2^-23 + the lse error
        assert float((m.sum(-1) - 1.0).abs().max()) < 1e-4
    with rt.use_compute_dtype(mode), torch.no_grad():
        some = enc.forward_features(x, output_attentions=True, attn_layers=(-1, 3))
        win = enc.forward_features(x, output_attentions=True, attn_layers=[5], attn_window=((0, 1), (1, 1 + N)))
        win2 = enc.forward_features(x, output_attentions=True, output_hidden_states=True, attn_layers=(0,), attn_window=((2, N), (3, N + 1)))
        hid = enc.forward_features(x, output_hidden_states=True)
    assert some.hidden_states is None and len(some.spatial_attentions) == 2 == len(some.temporal_attentions)       # in block order: 3, then 11
    assert torch.equal(some.spatial_attentions[0], out.spatial_attentions[3]) and torch.equal(some.spatial_attentions[1], out.spatial_attentions[11])
    assert torch.equal(some.temporal_attentions[0], out.temporal_attentions[3]) and torch.equal(some.temporal_attentions[1], out.temporal_attentions[11])
    assert len(win.spatial_attentions) == 1 and tuple(win.spatial_attentions[0].shape) == (B * T, H, 1, N)
    assert torch.equal(win.spatial_attentions[0], out.spatial_attentions[5][:, :, 0:1, 1:]) and torch.equal(win.temporal_attentions[0], out.temporal_attentions[5])
    assert torch.equal(win2.spatial_attentions[0], out.spatial_attentions[0][:, :, 2:N, 3:]) and len(win2.hidden_states) == DEPTH + 1
    assert hid.spatial_attentions is None and hid.temporal_attentions is None and len(hid.hidden_states) == DEPTH + 1
    assert all(torch.equal(a, b) for a, b in zip(hid.hidden_states, out.hidden_states))
    for o in (some, win, win2, hid):
        assert torch.equal(o.features, out.features)
    with pytest.raises(ValueError, match="attn_layers"), torch.no_grad():
        enc.forward_features(x, output_attentions=True, attn_layers=(12,))
    with pytest.raises(TypeError, match="forward_cls takes no"), torch.no_grad():
        enc.forward_cls(x, output_hidden_states=True)


@pytest.mark.parametrize("name", list(GEO))
@pytest.mark.parametrize("mode", MODES)
def test_features_are_bitwise_what_they_are_without_the_flags_eval(cases, full, mode, name):
    from alpro_amd import config as rt
    enc, x = cases(name)
    with rt.use_compute_dtype(mode), torch.no_grad():
        plain = enc.forward_features(x)
        sp = enc.forward_features(x, pooling="spatial")
        sp_o = enc.forward_features(x, pooling="spatial", output_attentions=True, output_hidden_states=True)
        vt = enc.model.forward_features(x, return_all_tokens=True)
        vt_o = enc.model.forward_features(x, return_all_tokens=True, output_attentions=True, output_hidden_states=True)
    assert torch.is_tensor(plain) and torch.equal(plain, full(name, mode).features)
    assert torch.equal(sp, sp_o.features) and torch.equal(vt, vt_o.features)
    assert all(torch.equal(a, b) for a, b in zip(vt_o.hidden_states + vt_o.temporal_attentions + sp_o.spatial_attentions,
                                                 full(name, mode).hidden_states + full(name, mode).temporal_attentions + full(name, mode).spatial_attentions))


def _streams():
    """What the next draws of the three random streams are: the dropout-seed counter, the device generator, the CPU generator."""
    from alpro_amd import config as rt
    return rt.dropout_state(), torch.rand(4, device="cuda").cpu(), torch.rand(4)


def _seed():
    from alpro_amd import config as rt
    torch.manual_seed(1234)
    rt.seed_dropout(99)


@pytest.mark.parametrize("name", list(GEO))
@pytest.mark.parametrize("mode", MODES)
def test_train_mode_no_grad_features_and_random_streams(cases, mode, name):
    from alpro_amd import config as rt
    enc, x = cases(name)
    B, T, N = _dims(name)
    enc.train()
    try:
        with rt.use_compute_dtype(mode), torch.no_grad():
            _seed()
            plain, s0 = enc.forward_features(x), _streams()
            _seed()
            out, s1 = enc.forward_features(x, output_attentions=True, output_hidden_states=True), _streams()
            _seed()
            rt.next_dropout_seed()
            other = enc.forward_features(x)
        assert s0[0][1] == 2 * DEPTH                                   # two dropout seeds per block were drawn
    finally:
        enc.eval()
    assert torch.equal(plain, out.features) and not torch.equal(plain, other)      # (another seed stream does change the features: the comparison sees dropout)
    assert s0[0] == s1[0] and torch.equal(s0[1], s1[1]) and torch.equal(s0[2], s1[2])
    assert len(out.spatial_attentions) == DEPTH and tuple(out.temporal_attentions[0].shape) == (B * N, H, T, T)
    for m in out.spatial_attentions + out.temporal_attentions:         # the softmax BEFORE dropout: no zeroed entries, rows sum to 1
        assert float((m.sum(-1) - 1.0).abs().max()) < 1e-4 and float(m.min()) > 0.0


def _anchored(enc, x, mode, probe, **flags):
    """One anchored forward + backward in train mode -> (features, {name: gradient}, random streams behind it, the output object or None)."""
    mp.fresh_grads(enc)
    _seed()
    keep = mp.arm_scale(mode)
    out = enc.forward_features(x, **flags)
    feats = out.features if flags else out
    assert feats.requires_grad
    mp.backward((feats * probe).sum(), mode)
    del keep
    grads = {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
    return feats.detach().clone(), grads, _streams(), (out if flags else None)


VARIANTS = ["plain", "recompute", "frozen_prefix", "unmerged"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(GEO))
@pytest.mark.parametrize("mode", MODES)
def test_anchored_path_features_gradients_and_streams_are_bitwise_unchanged(cases, monkeypatch, mode, name, variant):
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
    enc.train()
    try:
        for p in frozen:
            p.requires_grad_(False)
        with rt.use_compute_dtype(mode), rt.use_recompute(variant == "recompute"):
            f0, g0, s0, _ = _anchored(enc, x, mode, probe)
            f1, g1, s1, out = _anchored(enc, x, mode, probe, output_attentions=True, output_hidden_states=True)
    finally:
        enc.eval()
        for p in frozen:
            p.requires_grad_(True)
    assert torch.equal(f0, f1)
    assert g0.keys() == g1.keys() and len(g0) > (100 if variant != "frozen_prefix" else 80)
    assert not [n for n in g0 if not torch.equal(g0[n], g1[n])]
    if variant == "frozen_prefix":
        assert not [n for n in g0 if n.startswith(("model.blocks.0.", "model.blocks.1.", "model.patch_embed"))]
    assert s0[0] == s1[0] and s0[0][1] == 2 * DEPTH and torch.equal(s0[1], s1[1]) and torch.equal(s0[2], s1[2])
    assert len(out.hidden_states) == DEPTH + 1 and len(out.spatial_attentions) == DEPTH == len(out.temporal_attentions)
    assert all(tuple(m.shape) == (B * T, H, 1 + N, 1 + N) for m in out.spatial_attentions) and all(tuple(m.shape) == (B * N, H, T, T) for m in out.temporal_attentions)
    assert not any(t.requires_grad for t in out.hidden_states + out.spatial_attentions + out.temporal_attentions)
    for m in out.spatial_attentions + out.temporal_attentions:
        assert float((m.sum(-1) - 1.0).abs().max()) < 1e-4 and float(m.min()) > 0.0


@pytest.mark.parametrize("mode", MODES)
def test_sixteen_clips_collect_on_one_stream(cases, mode):
    """B = 16, T = 2, img 32 (N = 4, resampled position table): without flags the forward runs two half batches on two streams; with them it takes
    the one-stream loop, whose features are the one-stream forward's (config.set_split_streams(False)).  In fp16 this geometry takes the fused
    temporal launch (rows % 32 == 0, T = 2): q | k | v and the log-sum-exp rows are its training-form stores."""
    from alpro_amd import config as rt, hip
    enc, _ = cases("img48")
    geo = dict(img=32, T=2, B=16)
    x = pool_clips(geo).cuda()
    B, T, N = 16, 2, 4
    with rt.use_compute_dtype(mode), torch.no_grad():
        assert rt.split_streams(B)
        out = enc.forward_features(x, output_attentions=True, output_hidden_states=True)
        with rt.override(split_streams=False):
            one = enc.forward_features(x)
    assert torch.equal(out.features, one)
    assert tuple(out.temporal_attentions[0].shape) == (B * N, H, T, T) and tuple(out.spatial_attentions[-1].shape) == (B * T, H, 1 + N, 1 + N)
    for m in out.spatial_attentions + out.temporal_attentions:
        assert float((m.sum(-1) - 1.0).abs().max()) < 1e-4
    if mode == "fp16":
        assert hip.qkv_tattn_ok(torch.empty((B * N * T, D), dtype=torch.float16, device="cuda"), T)


def _ln64(x, ln):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), ln.weight.double(), ln.bias.double(), 1e-6)


def _lin64(x, lin):
    return x @ lin.weight.double().t() + lin.bias.double()


def _softmax_qk64(x, attn):
    """(groups, L, D) fp64 -> (softmax (groups, H, L, L), values (groups, H, L, 64)): vit.py:84-93."""
    G, L, _ = x.shape
    qkv = _lin64(x, attn.qkv).view(G, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    return torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * attn.scale, dim=-1), qkv[2]


@pytest.mark.parametrize("name", list(GEO))
@pytest.mark.parametrize("mode", MODES)
def test_every_map_against_an_fp64_restatement_of_its_block(cases, full, mode, name):
    """Block i restated in fp64 from hidden_states[i] (vit.py:146-180, eval mode): the temporal map needs temporal_norm1 and qkv only, the spatial
    map the whole temporal half first.  Limit: 2e-4 (fp32) / 8e-4 (fp16) of the map's largest element."""
    enc, _ = cases(name)
    B, T, N = _dims(name)
    out = full(name, mode)
    worst_t = worst_s = 0.0
    fails = []
    with torch.no_grad():
        for i, blk in enumerate(enc.model.blocks):
            x = out.hidden_states[i].double()
            xt = x[:, 1:].reshape(B * N, T, D)                                        # 'b (n t) m -> (b n) t m'
            p_t, v_t = _softmax_qk64(_ln64(xt, blk.temporal_norm1), blk.temporal_attn)
            a_t = (p_t @ v_t).transpose(1, 2).reshape(B * N, T, D)
            res_t = _lin64(_lin64(a_t, blk.temporal_attn.proj), blk.temporal_fc)
            xt = x[:, 1:] + res_t.reshape(B, N * T, D)
            cls = x[:, :1].repeat(1, T, 1).reshape(B * T, 1, D)                        # the clip's CLS token in front of every frame
            xs = xt.reshape(B, N, T, D).transpose(1, 2).reshape(B * T, N, D)           # 'b (n t) m -> (b t) n m'
            p_s, _ = _softmax_qk64(_ln64(torch.cat([cls, xs], 1), blk.norm1), blk.attn)
            for kind, ref, got in (("temporal", p_t, out.temporal_attentions[i]), ("spatial", p_s, out.spatial_attentions[i])):
                e, lim = float((got.double() - ref).abs().max()), MAP_TOL[mode] * float(ref.max())
                if kind == "temporal":
                    worst_t = max(worst_t, e / lim)
                else:
                    worst_s = max(worst_s, e / lim)
                if e > lim:
                    fails.append((kind, i, e, lim))
    print("\n[vit maps vs fp64 %s %s] worst error / limit: temporal %.3f, spatial %.3f" % (mode, name, worst_t, worst_s))
    assert not fails, fails


@pytest.mark.parametrize("name", list(GEO))
@pytest.mark.parametrize("mode", MODES)
def test_cls_rows_of_the_hidden_states(cases, full, mode, name):
    """The last hidden state through the final norm and the pooling IS `features`; and with the precise-CLS chain forced onto its side stream the
    CLS rows of every hidden state are those of a run with the chain on the launch stream (a copy taken before the chain is joined would hold the
    16-bit CLS row, or a torn one)."""
    from alpro_amd import config as rt, hip
    from alpro_amd.modeling.timesformer import vit
    enc, x = cases(name)
    B, T, N = _dims(name)
    out = full(name, mode)
    m = enc.model
    with torch.no_grad():
        direct, _ = hip.vit_final_pool(out.hidden_states[-1].clone(), m.norm.weight, m.norm.bias, vit.VIT_EPS, B, T, N, torch.float32)
    assert torch.equal(direct, out.features)
    runs = {}
    for v in ("1", "0"):
        with rt.override(cls_stream=v), rt.use_compute_dtype(mode), torch.no_grad():
            runs[v] = enc.forward_features(x, output_hidden_states=True)
    assert torch.equal(runs["1"].features, runs["0"].features)
    for i in range(DEPTH + 1):
        assert torch.equal(runs["1"].hidden_states[i][:, 0], runs["0"].hidden_states[i][:, 0]), "CLS rows of hidden state %d" % i
        assert torch.equal(runs["1"].hidden_states[i], runs["0"].hidden_states[i])
    if mode == "fp16":     # precise CLS rows are on: the CLS row of a block output is NOT the 16-bit graph's
        with rt.use_compute_dtype(mode), rt.use_cls_precise(False), torch.no_grad():
            plain16 = enc.forward_features(x, output_hidden_states=True)
        assert not torch.equal(plain16.hidden_states[1][:, 0], runs["1"].hidden_states[1][:, 0])


@pytest.mark.parametrize("name", list(GEO))
@pytest.mark.parametrize("mode", MODES)
def test_grounding_helpers(cases, full, mode, name):
    """Both helpers against the head mean and layer mean of the full maps' slices.  The helper averages the same fp32 numbers (12 heads, then 3
    layers, values in [0, 1]) but reduces a window tensor where this test reduces a strided slice, so the two sums may associate differently:
    15 additions of at most 2^-24 relative each on values <= 1 -- limit 1e-6."""
    from alpro_amd import config as rt
    from alpro_amd.grounding import frame_patch_attention, patch_temporal_attention
    enc, x = cases(name)
    B, T, N = _dims(name)
    g = int(round(N ** 0.5))
    out = full(name, mode)
    clips = x.transpose(1, 2).contiguous()                                             # (B, T, C, H, W), as the models take them
    holder = torch.nn.Module()
    holder.visual_encoder = enc
    layers = (-1, 0, 5)
    with rt.use_compute_dtype(mode):
        fp = frame_patch_attention(holder, clips, layers=layers)
        pt = patch_temporal_attention(enc, clips, layers=layers)
        last = frame_patch_attention(enc, clips)
    want_fp = sum(out.spatial_attentions[l][:, :, 0, 1:].mean(dim=1) for l in layers) / 3.0
    want_pt = sum(out.temporal_attentions[l].mean(dim=1) for l in layers) / 3.0
    assert tuple(fp.shape) == (B, T, g, g) and tuple(pt.shape) == (B, g, g, T, T) and fp.dtype == torch.float32
    assert float((fp - want_fp.view(B, T, g, g)).abs().max()) <= 1e-6 and float((pt - want_pt.view(B, g, g, T, T)).abs().max()) <= 1e-6
    assert float((last - out.spatial_attentions[-1][:, :, 0, 1:].mean(dim=1).view(B, T, g, g)).abs().max()) <= 1e-6
    assert float(fp.sum((-1, -2)).max()) < 1.0 and float(fp.min()) > 0.0              # not renormalised: the CLS key's share is left out
    assert float((pt.sum(-1) - 1.0).abs().max()) < 1e-4
    enc.train()
    try:
        with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
            frame_patch_attention(enc, clips)
        with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
            patch_temporal_attention(holder, clips)
    finally:
        enc.eval()
