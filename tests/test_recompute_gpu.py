"""Recomputing the ViT blocks' activations in backward (alpro_amd.config.recompute_blocks).

The oracle of every test is the switch-off run of the same build on the same inputs and seeds, and the bound is equality of bits: the replay
launches the forward kernels of the first pass once more on the same operands, every one of them deterministic.  The memory test asks for
peak(on) <= 0.5 * peak(off): kept (~3 KB per row and block) + one live block (~37 KB per row) + the backward's transients give 0.2-0.3 of
12 blocks x 37 KB, and a dict that survives its block's backward breaks the bound."""
import gc
import os

import numpy as np
import pytest
import torch

from tests.test_frozen_params_gpu import _freeze, _unfreeze
from tests.test_hip_ops import rnd
from tests.test_host_cpu import VENC, make_cfg
from tests.test_vit_attn_dropout import D, _block, _fix_drop_path

pytestmark = pytest.mark.gpu


# ---- 1. one block: forward_train -> slim -> replay ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
@pytest.mark.parametrize("B,T,W", [(2, 2, 4), (2, 3, 3)])   # block-diagonal temporal kernels | windowed ones
def test_block_replay_rebuilds_the_saved_dict_bit_for_bit_and_draws_nothing(B, T, W, mode):
    from alpro_amd import config as rt
    from alpro_amd.modeling.timesformer import vit
    N = W * W
    blk = _block(0.1)
    masks = _fix_drop_path(blk, B, T, N)
    assert float(masks[B][1]) == 0.0
    x = rnd(B, 1 + N * T, D, seed=800 + T).cuda()
    rt.seed_dropout(4242)
    with rt.use_compute_dtype(mode), torch.no_grad():
        out, sv = blk.forward_train(x.clone(), B, T, W)
        vit.join_cls_chain(out.device)
        torch.cuda.synchronize()
        assert sv["attn_drop"][1] and sv["attn_drop"][3]
        ref = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sv.items()}
        slim = vit.Block.slim_saved(sv)
        sv.clear()
    drop_state, cpu_rng, gpu_rng = list(rt.dropout_state()), torch.get_rng_state(), torch.cuda.get_rng_state()
    blk._drop = None                  # the replay may not ask for a mask ...
    blk._presampled = {B: None}       # ... nor look at the pre-sampled ones
    blk.eval()                        # ... nor read the module's mode
    with torch.no_grad():             # (outside use_compute_dtype: the dtype is the kept one)
        got = blk.replay(slim, W, cls_precise=rt.cls_precise(ref["dt"]))
    torch.cuda.synchronize()
    assert blk._presampled == {B: None}
    assert list(rt.dropout_state()) == drop_state
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(), gpu_rng)
    assert set(got) == set(ref)
    rows_t = B * N * T
    # lse_t is (ceil(rows / 32), H, 32), row r at [r // 32, :, r % 32]: behind the last row the buffer is torch.empty's memory, which no kernel
    # writes or reads (T = 3: 54 rows of 64 slots) -- every slot that holds a value is compared, every other tensor as a whole
    written = lambda t: t.permute(0, 2, 1).reshape(-1, t.shape[1])[:rows_t]   # noqa: E731
    for k, v in ref.items():
        if k == "lse_t":
            assert got[k].dtype == v.dtype and got[k].shape == v.shape and torch.equal(written(got[k]), written(v)), k
        elif torch.is_tensor(v):
            assert got[k].dtype == v.dtype and got[k].shape == v.shape and torch.equal(got[k], v), k
        else:
            assert got[k] == v, k
    assert got["x"] is slim["x"]


# ---- 2. / 3. the encoder under autograd ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc():
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    torch.manual_seed(5)
    e = TimeSformer(dict(VENC, num_frm=2, img_size=64, attn_drop_rate=0.1), input_format="RGB").cuda()
    with torch.no_grad():
        for blk in e.model.blocks:
            blk.temporal_fc.weight.normal_(0, 0.02)      # (zero-initialised behind block 0: give the temporal branch something to do)
    return e.train()


def _enc_step(e, x, dout, mode, recompute, pooling="temporal"):
    """forward_features under autograd + backward -> everything the contract names."""
    from alpro_amd import config as rt
    from tests.test_model_parity import arm_scale, backward
    for p in e.parameters():
        p.grad = None
    torch.manual_seed(77)
    rt.seed_dropout(77)
    with rt.use_compute_dtype(mode), rt.use_recompute(recompute):
        keep = arm_scale(mode)
        out = e.forward_features(x, pooling=pooling)
        assert out.requires_grad
        backward((out * dout).sum(), mode)
        del keep
    torch.cuda.synchronize()
    rt.set_armed_loss_scaler(None)
    grads = {n: (None if p.grad is None else p.grad.clone()) for n, p in e.named_parameters()}
    return dict(out=out.detach().clone(), grads=grads, drop=list(rt.dropout_state()), cpu=torch.get_rng_state(), gpu=torch.cuda.get_rng_state())


def _same_step(a, b, what):
    assert torch.equal(a["out"], b["out"]), what
    assert bool(torch.isfinite(a["out"]).all())
    assert a["drop"] == b["drop"], (what, a["drop"], b["drop"])
    assert torch.equal(a["cpu"], b["cpu"]) and torch.equal(a["gpu"], b["gpu"]), what
    assert [n for n in a["grads"] if (a["grads"][n] is None) != (b["grads"][n] is None)] == [], what
    bad = [n for n, g in a["grads"].items() if g is not None and not torch.equal(g, b["grads"][n])]
    assert not bad, (what, len(bad), bad[:4])
    assert all(bool(torch.isfinite(g).all()) for g in a["grads"].values() if g is not None), what


def _enc_inputs(pooling="temporal"):
    x = rnd(2, 3, 2, 64, 64, seed=810).cuda()            # 2 clips x 2 frames x 16 patches: the three drop-path row counts differ (32, 4, 2)
    rows = {"temporal": 1 + 16, "spatial": 1 + 2}[pooling]
    return x, rnd(2, rows, D, seed=811, scale=1e-2).cuda()


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_encoder_step_is_bitwise_the_stored_activation_step(enc, mode):
    """Default side streams: weight gradients on their side stream in the 16-bit mode, precise CLS (fp16, `auto`) on the launch stream."""
    from alpro_amd import config as rt
    assert rt.wgrad_stream_enabled() and not rt.recompute_blocks()
    x, dout = _enc_inputs()
    off = _enc_step(enc, x, dout, mode, False)
    assert off["drop"][1] == 24                           # two seeds per block were drawn
    assert all(g is not None and float(g.abs().sum()) > 0 for n, g in off["grads"].items() if not n.startswith("model.head"))
    on = _enc_step(enc, x, dout, mode, True)
    _same_step(on, off, mode)
    _same_step(_enc_step(enc, x, dout, mode, False), off, mode + ", off again")


@pytest.mark.parametrize("variant", ["wgrad_stream_off", "fused_temporal_training_form", "cls_side_stream", "pooling_spatial"])
def test_encoder_step_fp16_variants(enc, variant):
    from alpro_amd import config as rt
    pooling = "spatial" if variant == "pooling_spatial" else "temporal"
    x, dout = _enc_inputs(pooling)
    with rt.override("wgrad_stream", "fuse_temporal_attention", "cls_stream"):
        if variant == "wgrad_stream_off":
            rt.set_wgrad_stream(False)
        elif variant == "fused_temporal_training_form":
            rt.set_fuse_temporal_attention("1")
        elif variant == "cls_side_stream":
            rt.set_cls_stream("1")                         # the precise-CLS chain of the training forward -- and of the replay -- on its side stream
        off = _enc_step(enc, x, dout, "fp16", False, pooling)
        on = _enc_step(enc, x, dout, "fp16", True, pooling)
    _same_step(on, off, variant)


def test_encoder_step_with_frozen_subsets(enc, monkeypatch):
    """Embedding and blocks 0-1 frozen (the prefix: they run the no-grad forward and are never replayed), block 5 with frozen weights and
    trainable biases.  bf16: the third operand mode of the contract."""
    from alpro_amd import hip
    x, dout = _enc_inputs()
    _unfreeze(enc)
    _enc_step(enc, x, dout, "bf16", False)                # (operand caches are built outside the counted runs)
    names = ["model.patch_embed.", "model.cls_token", "model.pos_embed", "model.time_embed", "model.blocks.0.", "model.blocks.1."]
    names += ["model.blocks.5." + n for n, p in enc.model.blocks[5].named_parameters() if p.dim() == 2]
    frozen = set(_freeze(enc, names))
    calls = dict(tn=0)
    real_tn = hip.gemm_tn_acc

    def tn(*a, **k):
        calls["tn"] += 1
        return real_tn(*a, **k)

    replays = []
    for j, blk in enumerate(enc.model.blocks):
        real = blk.replay
        monkeypatch.setattr(blk, "replay", lambda *a, _real=real, _j=j, **k: (replays.append(_j), _real(*a, **k))[1])
    monkeypatch.setattr(hip, "gemm_tn_acc", tn)
    try:
        off = _enc_step(enc, x, dout, "bf16", False)
        n_off, calls["tn"] = calls["tn"], 0
        assert replays == []
        on = _enc_step(enc, x, dout, "bf16", True)
        n_on = calls["tn"]
    finally:
        _unfreeze(enc)
    assert replays == list(range(11, 1, -1)), replays
    _same_step(on, off, "frozen subsets")
    assert [n for n in frozen if on["grads"][n] is not None] == []
    assert all(on["grads"][n] is not None for n in on["grads"] if n not in frozen and not n.startswith("model.head"))
    # six weight-gradient GEMMs per block with trainable weights (fc2, fc1, spatial proj, spatial qkv, merged temporal projection, temporal qkv): nine
    # such blocks, none for block 5, the prefix or the embedding -- in the replayed step as in the stored one
    assert n_off == 6 * 9 and n_on == n_off, (n_off, n_on)


# ---- 4. whole models: fp16, FlatAdamW.backward ------------------------------------------------------------------------------------------------
def _model_steps(m, batch, loss_of):
    """One flat-buffer-building step, then the same training step with the switch off, on, off -> [(loss, flat gradient buffer)] * 3."""
    from alpro_amd import amp, config as rt
    from alpro_amd.optim import FlatAdamW
    n_scalers = len(amp._SCALERS)
    res = []
    m.train()
    try:
        with rt.use_compute_dtype("fp16"):
            for p in m.parameters():
                p.grad = None
            opt = FlatAdamW([p for p in m.parameters() if p.requires_grad], lr=0.0, weight_decay=0.0, allreduce=False)
            opt.scaler.to("cuda").state[0] = 1024.0
            torch.manual_seed(3)
            opt.backward(loss_of(m(batch))); opt.step(); opt.zero_grad()      # builds the flat buffers (lr = 0: the values stay)
            for flag in (False, True, False):
                opt.scaler.to("cuda").state[0] = 1024.0
                torch.manual_seed(9)
                rt.seed_dropout(9)
                with rt.use_recompute(flag):
                    loss = loss_of(m(batch))
                    opt.backward(loss)
                torch.cuda.synchronize()
                res.append((loss.detach().clone(), opt.flat["g"].clone()))
                opt.zero_grad()
    finally:
        m.eval()
        for p in m.parameters():
            p.grad = None
        del amp._SCALERS[n_scalers:]
        rt.set_armed_loss_scaler(None)
    return res


def _check_model(res, what):
    (l0, g0), (l1, g1), (l2, g2) = res
    assert bool(torch.isfinite(l0).all()) and bool(torch.isfinite(g0).all()) and float(g0.abs().sum()) > 0, what
    assert torch.equal(l2, l0) and torch.equal(g2, g0), what + ": the stored step does not repeat itself"
    assert torch.equal(l1, l0), (what, float(l1), float(l0))
    assert torch.equal(g1, g0), (what, int((g1 != g0).sum()), float((g1 - g0).abs().max()))


def test_retrieval_model_training_step(bert_cfg):
    from alpro_amd import config as rt
    from tests.golden import parity_cases as pc
    assert rt.text_stream_enabled()
    m, batch, _ = pc.build_case("retrieval_T2", bert_cfg, VENC, make_cfg, "cuda")
    _check_model(_model_steps(m, batch, lambda o: o["itm_loss"] + o["itc_loss"]), "retrieval")


def test_video_qa_model_training_step(bert_cfg):
    from tests.test_qa_parity import _qa_batch, _qa_model
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qa_T16_B2.npz"))
    m, batch = _qa_model(bert_cfg, 16), _qa_batch(2, 16, "qa_T16", g["labels"])
    _check_model(_model_steps(m, batch, lambda o: o["loss"]), "video QA")


# ---- 5. / 6. memory ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc4():
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    torch.manual_seed(6)
    return TimeSformer(dict(VENC, num_frm=4), input_format="RGB").cuda().train()


def _activation_peak(e, x, dout, recompute):
    from alpro_amd import config as rt
    from tests.test_model_parity import arm_scale, backward
    for p in e.parameters():
        p.grad = None
    with rt.use_compute_dtype("fp16"), rt.use_recompute(recompute):
        keep = arm_scale("fp16")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = e.forward_features(x)
        backward((out * dout).sum(), "fp16")
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out, keep
    rt.set_armed_loss_scaler(None)
    for p in e.parameters():
        p.grad = None
    return peak


def test_activation_peak_is_at_most_half_of_the_stored_step(enc4):
    """B = 4 x 4 frames x 224^2 (3140 token rows), fp16.  Measured on an MI355X: see DESIGN.md section 4.10."""
    x, dout = rnd(4, 3, 4, 224, 224, seed=820).cuda(), rnd(4, 197, D, seed=821, scale=1e-2).cuda()
    _activation_peak(enc4, x, dout, False)                # warm-up: operand copies, workspaces, side streams
    _activation_peak(enc4, x, dout, True)
    off = _activation_peak(enc4, x, dout, False)
    on = _activation_peak(enc4, x, dout, True)
    print("[recompute memory] activation peak, B = 4 x 4 frames x 224^2 fp16: switch off %.1f MiB, switch on %.1f MiB (ratio %.3f, limit 0.5)"
          % (off / 2 ** 20, on / 2 ** 20, on / off))
    assert on <= 0.5 * off, (on, off)


def test_a_run_whose_backward_is_never_called_releases_everything(enc4):
    """Forward under autograd, output dropped: what the run kept goes with it.  Counted in the bytes that were asked for ("requested_bytes"):
    memory_allocated() counts the allocator's blocks, and the one tensor the encoder holds from call to call (the patch rows of the last
    embedding) comes back in a block that is rounded differently from call to call (2420736 / 2586624 bytes for its 2408448)."""
    from alpro_amd import config as rt
    x = rnd(2, 3, 4, 224, 224, seed=822).cuda()
    live = lambda: torch.cuda.memory_stats()["requested_bytes.all.current"]   # noqa: E731
    for flag in (True, False):
        with rt.use_compute_dtype("fp16"), rt.use_recompute(flag):
            out = enc4.forward_features(x)                # warm-up (what the encoder keeps across calls exists afterwards)
            del out
            gc.collect()
            torch.cuda.synchronize()
            base, base_blocks = live(), torch.cuda.memory_allocated()
            out = enc4.forward_features(x)
            assert out.requires_grad and live() > base + 12 * x.shape[0] * 785 * D * 4 * (0 if flag else 1)
            del out
            gc.collect()
            torch.cuda.synchronize()
            print("[recompute release] switch %d: requested bytes %+d, allocator blocks %+d" % (flag, live() - base, torch.cuda.memory_allocated() - base_blocks))
            assert live() == base, (flag, live() - base)
