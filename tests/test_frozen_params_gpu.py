"""Frozen parameters (requires_grad == False) in the hand-written backward: `.grad is None`, no hidden work, the frozen prefix of an encoder.

The oracle is always the same module with everything trainable, run in the same process on the same inputs, drop-path scales and dropout
seeds.  Where the forward path does not change (scattered freezing inside one block / layer) outputs and every trainable gradient must be
BITWISE what the all-trainable run gives: the reductions are fixed-order.  Where a frozen prefix swaps Block.forward_train for Block.forward
the bound is the one tests/test_vit_block_paths.py holds between those two, accumulated over the prefix depth."""
import os

import numpy as np
import pytest
import torch

from tests.test_hip_ops import rnd
from tests.test_host_cpu import VENC, make_cfg
from tests.test_vit_attn_dropout import D, _block, _fix_drop_path

pytestmark = pytest.mark.gpu

TOL = {"fp32": 2e-4, "fp16": 8e-4, "bf16": 6e-3}          # tests/test_model_parity.py block tolerances (test_vit_block_paths.py: 2 * TOL * max|out| per block)
LOGIT_TOL = {"fp32": 1e-3, "fp16": 2e-3, "bf16": 1.6e-2}  # tests/test_model_parity.py: the logit / loss tolerance of every model-level comparison
GRAD_REL = 1e-3                                           # DESIGN section 2, "fused temporal launch on / off": |g - g_ref| <= 1e-3 |g_ref| per tensor


def _freeze(mod, names):
    """Freeze the parameters whose name starts with one of `names` (exact name, or a module prefix ending in '.'); returns them."""
    hit = [n for n, _ in mod.named_parameters() if any(n == k or (k.endswith(".") and n.startswith(k)) for k in names)]
    assert hit, names
    hs = set(hit)
    for n, p in mod.named_parameters():
        p.requires_grad_(n not in hs)
    return hit


def _unfreeze(mod):
    for p in mod.parameters():
        p.requires_grad_(True)


# ---- scattered freezing inside ONE ViT block ----------------------------------------------------------------------------------------------------
def _run_block(blk, x, dout, B, T, W, mode):
    from alpro_amd import config as rt
    for p in blk.parameters():
        p.grad = None
    rt.seed_dropout(4242)
    with rt.use_compute_dtype(mode), torch.no_grad():
        out, sv = blk.forward_train(x.clone(), B, T, W)
        dx, _ = blk.backward(sv, dout.clone())
    torch.cuda.synchronize()
    return out.clone(), dx.clone(), {n: (None if p.grad is None else p.grad.clone()) for n, p in blk.named_parameters()}


BLOCK_SETS = {
    "one_weight": ["mlp.fc1.weight"], "one_bias": ["attn.proj.bias"], "one_norm": ["norm1."], "temporal_norm": ["temporal_norm1."],
    "temporal_fc": ["temporal_fc."], "temporal_proj": ["temporal_attn.proj."], "temporal_fc_and_proj": ["temporal_fc.", "temporal_attn.proj."],
    "temporal_proj_bias_only_trainable": ["temporal_fc.", "temporal_attn.proj.weight"], "every_weight": None, "gamma_only": ["norm2.weight"],
}


@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,W", [(2, 2, 4), (2, 3, 3)])
def test_block_scattered_freezing_is_bitwise_the_all_trainable_run(B, T, W, mode, merge):
    N = W * W
    blk = _block(0.0)
    blk.merge_temporal_proj = merge
    _fix_drop_path(blk, B, T, N)
    x, dout = rnd(B, 1 + N * T, D, seed=700 + T).cuda(), rnd(B, 1 + N * T, D, seed=701 + T).cuda()
    _unfreeze(blk)
    out0, dx0, g0 = _run_block(blk, x, dout, B, T, W, mode)
    assert all(g is not None for g in g0.values())
    for tag, names in BLOCK_SETS.items():
        frozen = _freeze(blk, names if names is not None else [n for n, p in blk.named_parameters() if p.dim() == 2])
        out, dx, g = _run_block(blk, x, dout, B, T, W, mode)
        assert [n for n in frozen if g[n] is not None] == [], (tag, "a frozen parameter received a gradient")
        assert torch.equal(out, out0) and torch.equal(dx, dx0), (tag, float((dx - dx0).abs().max()))
        bad = [n for n in g0 if n not in frozen and not torch.equal(g[n], g0[n])]
        assert not bad, (tag, bad, float((g[bad[0]] - g0[bad[0]]).abs().max()))
    _unfreeze(blk)


# ---- scattered freezing inside ONE BERT layer ---------------------------------------------------------------------------------------------------
def _bert_layer():
    import types
    from alpro_amd.modeling.xbert import BertLayer
    from tests.conftest import BERT_CFG
    cfg = types.SimpleNamespace(**dict(BERT_CFG, chunk_size_feed_forward=0))     # hidden / attention dropout 0.1: the layer's own train-mode form
    torch.manual_seed(3)
    layer = BertLayer(cfg, 0)
    with torch.no_grad():
        for p in layer.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.3)
    return layer.cuda().train()


def _run_layer(layer, h32, do32, kb, B, L, mode):
    from alpro_amd import config as rt
    for p in layer.parameters():
        p.grad = None
    rt.seed_dropout(99)
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[mode]
    with rt.use_compute_dtype(mode), torch.no_grad():
        o32, o_t, sv = layer.forward_train(h32, h32.to(dt), kb, B, L)
        d32, d_t = layer.backward(sv, do32.clone(), None)
    torch.cuda.synchronize()
    return o32.clone(), d32.clone(), d_t.clone(), {n: (None if p.grad is None else p.grad.clone()) for n, p in layer.named_parameters()}


LAYER_SETS = {
    "one_weight": ["intermediate.dense.weight"], "one_bias": ["output.dense.bias"], "one_norm": ["attention.output.LayerNorm."],
    "q_third": ["attention.self.query."], "k_third": ["attention.self.key."], "v_weight": ["attention.self.value.weight"], "every_weight": None,
}


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("L", [8, 40])
def test_bert_layer_scattered_freezing_is_bitwise_the_all_trainable_run(L, mode):
    B = 2
    layer = _bert_layer()
    h32, do32 = rnd(B * L, D, seed=710).cuda(), rnd(B * L, D, seed=711).cuda()
    mask = torch.ones(B, L)
    mask[1, L - 3:] = 0                                   # a key bias: the second caption is padded
    kb = ((1.0 - mask) * -10000.0).cuda().contiguous()
    ref = _run_layer(layer, h32, do32, kb, B, L, mode)
    assert all(g is not None for g in ref[3].values())
    for tag, names in LAYER_SETS.items():
        frozen = _freeze(layer, names if names is not None else [n for n, p in layer.named_parameters() if p.dim() == 2])
        got = _run_layer(layer, h32, do32, kb, B, L, mode)
        assert [n for n in frozen if got[3][n] is not None] == [], tag
        for a, b in zip(got[:3], ref[:3]):
            assert torch.equal(a, b), tag
        bad = [n for n in ref[3] if n not in frozen and not torch.equal(got[3][n], ref[3][n])]
        assert not bad, (tag, bad)
    _unfreeze(layer)


# ---- no hidden work ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_frozen_linears_and_norms_launch_nothing_for_their_gradients(mode, monkeypatch):
    """Every weight of the block frozen, biases and norms trainable: no weight-gradient GEMM runs -- neither alpro_gemm_tn_acc nor, in fp32, a
    transpose that feeds one (the biases take their column sums from alpro_colsum_tn / a plain sum) -- and every bias and norm still gets its
    gradient.  The same with the biases frozen too.  All four norms frozen: every LayerNorm backward of the block is called with dgamma = dbeta = None
    (the data-only kernel: no column sums, no colsum_reduce launch), except norm1's under the merged projection while temporal_fc.bias still
    wants its column sums -- frozen too, that one is data-only as well."""
    from alpro_amd import hip
    B, T, W = 2, 2, 4
    N = W * W
    blk = _block(0.0)
    _fix_drop_path(blk, B, T, N)
    x, dout = rnd(B, 1 + N * T, D, seed=720).cuda(), rnd(B, 1 + N * T, D, seed=721).cuda()
    calls = dict(tn=0, tr=0, ln=[])
    real_tn, real_tr, real_ln = hip.gemm_tn_acc, hip.transpose, hip.layernorm_bwd

    def tn(*a, **k):
        calls["tn"] += 1
        return real_tn(*a, **k)

    def trp(*a, **k):
        calls["tr"] += 1
        return real_tr(*a, **k)

    def ln(dy, x_, gamma, eps, dx, dgamma=None, dbeta=None, **k):
        calls["ln"].append((dgamma is None, dbeta is None, (k.get("emit") or {}).get("colsum_pre") is None))
        return real_ln(dy, x_, gamma, eps, dx, dgamma, dbeta, **k)

    _unfreeze(blk)
    _run_block(blk, x, dout, B, T, W, mode)              # (operand caches -- W^T, the merged projection -- are built outside the counted run)
    monkeypatch.setattr(hip, "gemm_tn_acc", tn)
    monkeypatch.setattr(hip, "transpose", trp)
    monkeypatch.setattr(hip, "layernorm_bwd", ln)
    _run_block(blk, x, dout, B, T, W, mode)
    assert (calls["tn"] if mode != "fp32" else calls["tr"]) > 0 and len(calls["ln"]) == 3 and not any(c[0] or c[1] for c in calls["ln"])
    for names in ([n for n, p in blk.named_parameters() if p.dim() == 2], [n for n, _ in blk.named_parameters() if "norm" not in n]):
        frozen = _freeze(blk, names)
        calls.update(tn=0, tr=0, ln=[])
        _, _, g = _run_block(blk, x, dout, B, T, W, mode)
        assert calls["tn"] == 0 and calls["tr"] == 0, calls
        assert all(g[n] is None for n in frozen) and all(g[n] is not None and float(g[n].abs().sum()) > 0 for n in g if n not in frozen)
    _freeze(blk, ["norm1.", "norm2.", "temporal_norm1."])
    calls.update(tn=0, tr=0, ln=[])
    _run_block(blk, x, dout, B, T, W, mode)
    # norm1 still serves temporal_fc.bias (colsum_pre given): the wrapper then runs the column-sum kernel into its throw-away pair
    assert len(calls["ln"]) == 3 and all(c[0] and c[1] for c in calls["ln"]) and sum(not c[2] for c in calls["ln"]) == 1, calls["ln"]
    for p in blk.parameters():
        p.requires_grad_(False)
    blk.mlp.fc1.weight.requires_grad_(True)
    calls.update(tn=0, tr=0, ln=[])
    _run_block(blk, x, dout, B, T, W, mode)
    assert all(c == (True, True, True) for c in calls["ln"]) and len(calls["ln"]) == 3, calls["ln"]
    assert calls["tn"] == (1 if mode != "fp32" else 0)
    _unfreeze(blk)


# ---- frozen prefixes on the smallest fixture model: the 2-frame retrieval geometry, B = 3 --------------------------------------------------
@pytest.fixture(scope="module")
def retrieval(bert_cfg):
    from tests.golden import parity_cases as pc
    m, batch, _ = pc.build_case("retrieval_T2", bert_cfg, VENC, make_cfg, "cuda")
    return m, batch


def _argmax_multinomial(w, n=1, *a, **k):
    return w.argmax(dim=-1, keepdim=True)


def _step(m, batch, mode, loss_of, monkeypatch):
    """One forward + backward; -> (outputs as float64 numpy, {name: grad clone or None}, the visual encoder's output)."""
    from alpro_amd import config as rt
    from tests.test_model_parity import arm_scale, backward
    for p in m.parameters():
        p.grad = None
    monkeypatch.setattr(torch, "multinomial", _argmax_multinomial)
    seen = {}
    ff = m.visual_encoder.forward_features

    def spy(*a, **k):
        seen["video"] = ff(*a, **k)
        return seen["video"]

    monkeypatch.setattr(m.visual_encoder, "forward_features", spy)
    rt.seed_dropout(7)
    torch.manual_seed(7)
    with rt.use_compute_dtype(mode):
        keep = arm_scale(mode)
        out = m(batch)
        gs = backward(loss_of(out), mode)
        del keep
    torch.cuda.synchronize()
    monkeypatch.setattr(m.visual_encoder, "forward_features", ff)
    grads = {n: (None if p.grad is None else (p.grad / gs).clone()) for n, p in m.named_parameters()}
    return {k: v.detach().double().cpu().numpy() for k, v in out.items() if torch.is_tensor(v) and v.is_floating_point()}, grads, seen["video"].detach().clone()


def _spy_blocks(mods, monkeypatch):
    """Count backward entries and SAVING forward_train entries of the given blocks / layers (a BERT layer's no-grad forward is
    forward_train(save=False), which keeps nothing for a backward and is not counted)."""
    hits = {}
    for i, b in enumerate(mods):
        for meth in ("forward_train", "backward"):
            real = getattr(b, meth)

            def wrapped(*a, _real=real, _key=(i, meth), **k):
                if _key[1] == "backward" or k.get("save", True):
                    hits[_key] = hits.get(_key, 0) + 1
                return _real(*a, **k)
            monkeypatch.setattr(b, meth, wrapped)
    return hits


VIT_EMB = ["visual_encoder.model.patch_embed.", "visual_encoder.model.cls_token", "visual_encoder.model.pos_embed", "visual_encoder.model.time_embed"]
TXT_EMB = ["text_encoder.bert.embeddings."]


def _prefix_sets(m):
    nb = len(m.visual_encoder.model.blocks)
    blocks = lambda k: ["visual_encoder.model.blocks.%d." % i for i in range(k)]   # noqa: E731
    heads = ("temp", "vision_proj.", "text_proj.", "itm_head.")
    return {
        "vit_emb_and_first_block": (VIT_EMB + blocks(1), 1, 0),
        "vit_emb_and_all_but_last_block": (VIT_EMB + blocks(nb - 1), nb - 1, 0),
        "whole_vit_text_trainable": (["visual_encoder."], nb, 0),
        "text_emb_and_first_layer": (TXT_EMB + ["text_encoder.bert.encoder.layer.0."], 0, 1),
        # the fusion layers have a prefix of their own only when neither embedding stream needs a gradient: both encoders and fusion layer 6 frozen
        "both_encoders_and_first_fusion_layer": (["visual_encoder."] + TXT_EMB + ["text_encoder.bert.encoder.layer.%d." % i for i in range(7)], nb, 7),
        "everything_but_the_heads": ([n for n, _ in m.named_parameters() if not n.startswith(heads)], nb, 12),
    }


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_frozen_prefix_skips_its_blocks_and_matches_the_all_trainable_step(retrieval, mode, monkeypatch):
    from alpro_amd import config as rt
    m, batch = retrieval
    loss_of = lambda out: out["itm_loss"] + out["itc_loss"]   # noqa: E731
    _unfreeze(m)
    out0, g0, vid0 = _step(m, batch, mode, loss_of, monkeypatch)
    vblocks, layers = list(m.visual_encoder.model.blocks), list(m.text_encoder.bert.encoder.layer)
    report = []
    for tag, (names, vdepth, tdepth) in _prefix_sets(m).items():
        for plain in (False, True):     # plain: fused temporal launch, split streams and the deferred temporal add switched off in the prefix
            if plain and vdepth == 0:
                continue
            frozen = set(_freeze(m, names))
            with monkeypatch.context() as mp:
                hits = _spy_blocks(vblocks + layers, mp)
                with rt.override(**(dict(fuse_temporal_attention="0", split_streams="0", defer_temporal_add=False) if plain else {})):
                    out, g, vid = _step(m, batch, mode, loss_of, mp)
            # frozen: no gradient; trainable: one
            assert [n for n in frozen if g[n] is not None] == [], tag
            missing = [n for n in g0 if n not in frozen and g0[n] is not None and g[n] is None]
            assert not missing, (tag, missing[:4])
            # the prefix blocks' / layers' saving forward and backward are never entered
            entered = [k for k in hits if (k[0] < vdepth) or (len(vblocks) <= k[0] < len(vblocks) + tdepth)]
            assert not entered, (tag, entered[:4])
            if tdepth == 12:    # every BERT layer frozen: the text pass has no backward; the fusion pass still carries d(video) ... unless the ViT is frozen too
                assert not [k for k in hits if k[1] == "backward"], tag
            # bounds: the visual encoder's output within depth * 2 * TOL * max|out| (test_vit_block_paths.py, per prefix block); losses / logits within the
            # model-level logit tolerance; every trainable gradient within 1e-3 of its norm
            lim_v = max(vdepth, 0) * 2 * TOL[mode] * float(vid0.abs().max())
            err_v = float((vid - vid0).abs().max())
            err_o = max(float(np.abs(out[k] - out0[k]).max()) for k in ("itc_loss", "itm_loss", "itm_scores"))
            worst, wname = 0.0, ""
            for n in g0:
                if n in frozen or g0[n] is None:
                    continue
                assert bool(torch.isfinite(g[n]).all()), (tag, n)
                r = float((g[n] - g0[n]).norm() / g0[n].norm().clamp_min(1e-20)) if float(g0[n].norm()) > 1e-12 else 0.0
                if r > worst:
                    worst, wname = r, n
            report.append((tag, plain, err_v, lim_v, err_o, worst, wname))
            print("[frozen prefix %s %s plain=%d] video-embeds err %.3e (limit %.3e)  loss/logit err %.3e (limit %.1e)  worst grad rel err %.3e at %s (limit %.0e)"
                  % (mode, tag, plain, err_v, lim_v, err_o, LOGIT_TOL[mode], worst, wname, GRAD_REL))
    _unfreeze(m)
    for tag, plain, err_v, lim_v, err_o, worst, wname in report:
        if plain:
            # measured: 0 in both modes and every set -- with the fused temporal launch, the split streams and the deferred add off the in-place forward
            # states the training forward's arithmetic kernel for kernel (on this 2-frame geometry the default path measured 0 as well, on the
            # 4-frame pretraining fixture it does not: test_pretraining_model_with_frozen_encoders), so the plain form is held to equality
            assert err_v == 0.0 and err_o == 0.0 and worst == 0.0, (tag, err_v, err_o, worst, wname)
        assert err_v <= lim_v, (tag, plain, err_v, lim_v)
        assert err_o <= LOGIT_TOL[mode], (tag, plain, err_o)
        assert worst <= GRAD_REL, (tag, plain, worst, wname)


def test_visual_encoder_frozen_step_peaks_below_the_all_trainable_step(retrieval, monkeypatch):
    m, batch = retrieval
    loss_of = lambda out: out["itm_loss"] + out["itc_loss"]   # noqa: E731
    peaks = {}
    for tag in ("warm", "all", "frozen"):
        _unfreeze(m)
        if tag == "frozen":
            _freeze(m, ["visual_encoder."])
        for p in m.parameters():
            p.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        _step(m, batch, "bf16", loss_of, monkeypatch)
        for p in m.parameters():
            p.grad = None
        peaks[tag] = torch.cuda.max_memory_allocated()
    _unfreeze(m)
    print("[frozen memory] peak all-trainable %.1f MB, visual encoder frozen %.1f MB" % (peaks["all"] / 2 ** 20, peaks["frozen"] / 2 ** 20))
    assert peaks["frozen"] < peaks["all"], peaks


# ---- train-mode stochasticity stays the reference's inside a frozen prefix -------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_vit():
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    torch.manual_seed(5)
    enc = TimeSformer(dict(VENC, num_frm=2, attn_drop_rate=0.1, drop_path_rate=0.2), input_format="RGB").cuda()
    with torch.no_grad():
        for blk in enc.model.blocks:
            blk.temporal_fc.weight.normal_(0, 0.02)      # (zero-initialised behind block 0: give the temporal branch something to do)
    return enc


def _visual_run(enc, x, mode, seed=31):
    from alpro_amd import config as rt
    from alpro_amd.modeling.timesformer.vit import _VisualRun
    run = _VisualRun(enc)
    rt.seed_dropout(seed)
    torch.manual_seed(seed)
    with rt.use_compute_dtype(mode), torch.no_grad():
        out = run.forward(x)
    torch.cuda.synchronize()
    return run, out


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_frozen_prefix_keeps_drop_path_attention_dropout_and_the_seed_stream(small_vit, mode):
    from alpro_amd import config as rt
    from alpro_amd.modeling.timesformer import vit
    enc, m, K = small_vit, small_vit.model, 3
    x = rnd(2, 3, 2, 64, 64, seed=730).cuda()            # 2 clips x 2 frames x 16 patches: the three drop-path row counts differ (32, 4, 2)
    enc.train()
    _unfreeze(enc)
    run_all, out_all = _visual_run(enc, x, mode)
    seeds_all = [sv["attn_drop"] for sv in run_all.saved]
    assert len(seeds_all) == 12 and all(s[1] and s[3] for s in seeds_all)
    _freeze(enc, ["model.patch_embed.", "model.cls_token", "model.pos_embed", "model.time_embed"] + ["model.blocks.%d." % i for i in range(K)])
    run_fro, out_fro = _visual_run(enc, x, mode)
    assert run_fro.nfro == K and len(run_fro.saved) == 12 - K
    # the suffix sees the seeds it sees without freezing
    assert [sv["attn_drop"] for sv in run_fro.saved] == seeds_all[K:]
    prefix_out = run_fro.saved[0]["x"].clone()
    # ... the prefix output is the train-mode no-grad forward of the unfrozen model (same masks, same seeds) ...
    _unfreeze(enc)
    rt.seed_dropout(31)
    torch.manual_seed(31)
    with rt.use_compute_dtype(mode), torch.no_grad():
        tok, T, W, N = m._embed(x)
        vit.sample_drop_paths(m.blocks, 2, T, N, tok.device)
        for blk in m.blocks[:K]:
            tok = blk(tok, 2, T, W)
        vit.join_cls_chain(tok.device)
        for blk in m.blocks:
            blk._presampled = None
        # ... and not its eval-mode forward
        enc.eval()
        tok_eval, _, _, _ = m._embed(x)
        for blk in m.blocks[:K]:
            tok_eval = blk(tok_eval, 2, T, W)
        vit.join_cls_chain(tok.device)
        enc.train()
    torch.cuda.synchronize()
    assert torch.equal(prefix_out, tok)
    assert float((prefix_out - tok_eval).abs().max()) > 1e-2 * float(tok_eval.abs().max())
    # the whole encoder's output stays within the forward / forward_train bound over K blocks
    err, lim = float((out_fro - out_all).abs().max()), K * 2 * TOL[mode] * float(out_all.abs().max())
    print("[frozen prefix train mode %s] output err %.3e limit %.3e" % (mode, err, lim))
    assert err <= lim
    enc.eval()
    for s in run_all.saved + run_fro.saved:
        s.clear()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_frozen_prefix_on_two_streams_applies_the_masks_drawn_for_the_step(small_vit, mode):
    """Drop-path only (no attention dropout): the prefix goes through run_blocks, and with the two half-batch streams switched on each half takes its
    rows of the masks sample_drop_paths drew for the whole batch -- the prefix output is the one-stream prefix output (same masks), not a fresh draw."""
    from alpro_amd import config as rt
    enc, K = small_vit, 3
    x = rnd(2, 3, 2, 64, 64, seed=731).cuda()
    drops = [d for blk in enc.model.blocks for d in (blk.attn.attn_drop, blk.temporal_attn.attn_drop)]
    enc.train()
    for d in drops:
        d.p = 0.0
    rates = [blk.drop_path.drop_prob for blk in enc.model.blocks[1:K]]
    for blk in enc.model.blocks[1:K]:
        blk.drop_path.drop_prob = 0.5                    # (the prefix blocks' own rates are 2-4 %: make a wrong mask show)
    _freeze(enc, ["model.patch_embed.", "model.cls_token", "model.pos_embed", "model.time_embed"] + ["model.blocks.%d." % i for i in range(K)])
    try:
        outs = {}
        for split in ("0", "1"):
            with rt.override(split_streams=split):
                run, _ = _visual_run(enc, x, mode)
            assert run.nfro == K
            outs[split] = run.saved[0]["x"].clone()
            for s_ in run.saved:
                s_.clear()
    finally:
        for d in drops:
            d.p = 0.1
        for blk, r in zip(enc.model.blocks[1:K], rates):
            blk.drop_path.drop_prob = r
        _unfreeze(enc)
        enc.eval()
    err, lim = float((outs["1"] - outs["0"]).abs().max()), K * 2 * TOL[mode] * float(outs["0"].abs().max())
    print("[frozen prefix two streams %s] prefix output, split against one stream: err %.3e limit %.3e" % (mode, err, lim))
    assert err <= lim


# ---- freezing for a step and unfreezing again on the same model and optimizer (fp16: FlatAdamW.backward with loss scaling) ------------------
def test_toggling_requires_grad_between_steps_on_one_flat_adamw(small_vit):
    """FlatAdamW built over all parameters while trainable.  Step 2 runs with block 0 frozen: nothing writes its slice of the flat gradient buffer
    (it keeps the zeros zero_grad left), and the optimizer leaves its value and moments alone -- what torch.optim does with `.grad is None` --
    although weight decay is on.  Step 3, unfrozen again: the gradients are those of a fresh all-trainable model holding the same values."""
    from alpro_amd import amp, config as rt
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    from alpro_amd.optim import FlatAdamW
    enc = small_vit
    enc.eval()                                            # (no stochasticity here: the comparison with the fresh model is then exact)
    n_scalers = len(amp._SCALERS)
    _unfreeze(enc)
    x = rnd(2, 3, 2, 64, 64, seed=740).cuda()
    loss_of = lambda e: e.forward_features(x).float().square().mean()   # noqa: E731
    blk0 = list(enc.model.blocks[0].parameters())
    with rt.use_compute_dtype("fp16"):
        for p in enc.parameters():
            p.grad = None
        opt = FlatAdamW([p for n, p in enc.named_parameters() if not n.startswith("model.head")], lr=1e-3, weight_decay=0.1, allreduce=False)
        opt.scaler.to("cuda").state[0] = 1024.0
        opt.backward(loss_of(enc)); opt.step(); opt.zero_grad()                       # step 1: all trainable (builds the flat buffers)
        assert all(p.grad is not None and p.grad.data_ptr() >= opt.flat["g"].data_ptr() for p in blk0)
        before_p = [p.detach().clone() for p in blk0]
        before_m = opt.flat["m"].clone()
        other = enc.model.blocks[5].mlp.fc1.weight
        other_before = other.detach().clone()
        for p in blk0:
            p.requires_grad_(False)
        opt.backward(loss_of(enc))                                                    # step 2: block 0 frozen
        torch.cuda.synchronize()
        assert all(float(p.grad.abs().sum()) == 0.0 for p in blk0), "something wrote a frozen parameter's gradient"
        assert float(other.grad.abs().sum()) > 0.0
        opt.step(); opt.zero_grad()
        torch.cuda.synchronize()
        assert all(torch.equal(p.detach(), b) for p, b in zip(blk0, before_p)), "a frozen parameter moved (weight decay on stale zeros?)"
        for p in blk0:
            a, e = opt._span[id(p)]
            assert torch.equal(opt.flat["m"][a:e], before_m[a:e])
        assert not torch.equal(other.detach(), other_before)
        for p in blk0:
            p.requires_grad_(True)
        opt.backward(loss_of(enc))                                                    # step 3: unfrozen again
        torch.cuda.synchronize()
        got = {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
        fresh = TimeSformer(dict(VENC, num_frm=2, attn_drop_rate=0.1, drop_path_rate=0.2), input_format="RGB").cuda().eval()
        fresh.load_state_dict({k: v.detach().clone() for k, v in enc.state_dict().items()})
        opt2 = FlatAdamW([p for n, p in fresh.named_parameters() if not n.startswith("model.head")], lr=0.0, allreduce=False)
        opt2.scaler.to("cuda").state[0] = float(opt.scaler.loss_scale())
        opt2.backward(loss_of(fresh))
        torch.cuda.synchronize()
        worst = 0.0
        for n, p in fresh.named_parameters():
            if p.grad is None:
                continue
            worst = max(worst, float((got[n] - p.grad).norm() / p.grad.norm().clamp_min(1e-20)))
        print("[toggling] step-3 gradients against a fresh all-trainable model: worst rel err %.3e (limit %.0e)" % (worst, GRAD_REL))
        assert all(float(got["model.blocks.0." + n].abs().sum()) > 0 for n, _ in enc.model.blocks[0].named_parameters())
        assert worst <= GRAD_REL
        opt.zero_grad()
    for p in enc.parameters():
        p.grad = None
    del amp._SCALERS[n_scalers:]                          # the two optimizers' loss scalers leave the process-wide registry with them
    rt.set_armed_loss_scaler(None)


# ---- the models end to end ---------------------------------------------------------------------------------------------------------------------
def _end_to_end(m, batch, mode, loss_of, monkeypatch, loss_keys):
    nb = len(m.visual_encoder.model.blocks)
    bert = "text_encoder.bert." if hasattr(m.text_encoder, "bert") else "text_encoder."
    own = lambda n: not n.startswith("prompter.")   # noqa: E731  (the frozen teacher of the pretraining model is not part of the comparison)
    _unfreeze(m)
    if hasattr(m, "prompter"):
        for p in m.prompter.parameters():
            p.requires_grad_(False)
    base_frozen = {n for n, p in m.named_parameters() if not p.requires_grad}
    out0, g0, _ = _step(m, batch, mode, loss_of, monkeypatch)
    sets = {"vit_frozen": ["visual_encoder."],
            "vit_half_and_text_embeddings": VIT_EMB + ["visual_encoder.model.blocks.%d." % i for i in range(nb // 2)] + [bert + "embeddings."]}
    for tag, names in sets.items():
        frozen = set(_freeze(m, names + sorted(base_frozen))) if base_frozen else set(_freeze(m, names))
        out, g, _ = _step(m, batch, mode, loss_of, monkeypatch)      # all side streams at their defaults
        assert [n for n in frozen if g[n] is not None] == [], tag
        for k in loss_keys:
            err = float(np.abs(out[k] - out0[k]).max())
            print("[frozen end to end %s %s %s] %s err %.3e (limit %.1e)" % (type(m).__name__, mode, tag, k, err, LOGIT_TOL[mode]))
            assert err <= LOGIT_TOL[mode], (tag, k, err)
        for n in g0:
            if n in frozen or g0[n] is None or not own(n):
                continue
            assert g[n] is not None and bool(torch.isfinite(g[n]).all()), (tag, n)
            if float(g0[n].abs().sum()) > 0:
                assert float(g[n].abs().sum()) > 0, (tag, n)
    _unfreeze(m)
    if hasattr(m, "prompter"):
        for p in m.prompter.parameters():
            p.requires_grad_(False)


@pytest.fixture(scope="module")
def pretrain_release(bert_cfg):
    from tests.golden import parity_cases as pc
    m, batch, _ = pc.build_case("pretrain_release_T4_L30", bert_cfg, VENC, make_cfg, "cuda")   # the released 4-frame x 30-token geometry
    return m, batch


@pytest.fixture(scope="module")
def qa16(bert_cfg):
    from tests.test_qa_parity import _qa_batch, _qa_model
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qa_T16_B2.npz"))
    return _qa_model(bert_cfg, 16), _qa_batch(2, 16, "qa_T16", g["labels"])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_pretraining_model_with_frozen_encoders(pretrain_release, mode, monkeypatch):
    m, batch = pretrain_release
    _end_to_end(m, batch, mode, lambda o: o["mlm_loss"] + o["itm_loss"] + o["itc_loss"] + o["mpm_loss"], monkeypatch, ("itc_loss", "itm_loss", "mlm_loss", "mpm_loss"))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_video_qa_model_with_frozen_encoders(qa16, mode, monkeypatch):
    m, batch = qa16
    _end_to_end(m, batch, mode, lambda o: o["loss"], monkeypatch, ("loss", "logits"))

