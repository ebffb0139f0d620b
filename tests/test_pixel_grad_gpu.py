"""GPU: the gradient of TimeSformer.forward_features with respect to the video pixels, and the two grounding helpers built on it.

The encoder alone, on the two small geometries of tests/golden/make_golden_pool_modes.py (img 64 x 3 frames, N = 16: the windowed temporal kernels;
img 48 x 2 frames, N = 9, odd), 2 clips, 12 blocks, clips from pool_clips and cotangents from pool_probe: x.grad against the fp64 oracle's
(tests/pixel_grad_cases.oracle_case), the 'none' pooling under the broadcast 'temporal' cotangent, and the bitwise invariances -- asking for the
pixel gradient changes no output, parameter gradient or random draw; freezing every parameter, recomputation, a collector and a second run change
no bit of it.  The full chain on the retrieval fixture model (2 frames at 224 px): grounding.pixel_gradient against AlproOracle.forward_inference
in fp64 with autograd to visual_inputs.

Limits, as a fraction of the largest reference magnitude: fp32 the project's exact-mode 2e-4, fp16 and bf16 the 1e-2 / 4e-2 that
tests/test_model_parity.py applies to gradients against the reference (test_pretrain_gradients_vs_reference), read from its parametrisation."""
import numpy as np
import pytest
import torch

from tests import pixel_grad_cases as pc
from tests import test_model_parity as mp
from tests.golden.make_golden_pool_modes import GEOMETRIES, pool_probe
from tests.test_model_parity import fixture_models  # noqa: F401  (the module-scoped fixture: the retrieval model is built once)
from tests.test_pool_modes_parity import arm_scale, scaled_backward

pytestmark = pytest.mark.gpu

_G = dict(mp.test_pretrain_gradients_vs_reference.pytestmark[0].args[1])
TOL = {"fp32": 2e-4, "fp16": _G["fp16"], "bf16": _G["bf16"]}
assert (TOL["fp16"], TOL["bf16"]) == (1e-2, 4e-2)
POOLINGS = pc.POOLINGS


@pytest.fixture(scope="module")
def cases():
    """geometry index -> (encoder in eval mode on the device, clips on the device, {pooling: (out64, dx64)}), built once."""
    built = {}

    def get(i):
        if i not in built:
            enc, x, ref = pc.oracle_case(i)
            built[i] = (enc.cuda().eval(), x.cuda(), ref)
        return built[i]
    return get


def run(enc, x, pooling, mode, x_grad=True, probe=None, seed=None, recompute=False, collect=False):
    """One forward and scaled backward from fresh gradients -> (out, x.grad / scale or None, {name: parameter gradient}, the dropout-seed counter)."""
    from alpro_amd import config as rt
    mp.fresh_grads(enc)
    if seed is not None:
        rt.seed_dropout(seed)
        torch.manual_seed(seed)
    xr = x.clone().requires_grad_(x_grad)
    with rt.use_compute_dtype(mode), rt.use_recompute(recompute):
        keep = arm_scale(mode, pooling)
        out = enc.forward_features(xr, return_all_tokens=True, pooling=pooling, **(dict(output_attentions=True, attn_layers=(0, -1)) if collect else {}))
        if collect:
            assert len(out.spatial_attentions) == 2 and len(out.temporal_attentions) == 2
            out = out.features
        gs = scaled_backward(out, pool_probe(pooling, out.shape).cuda() if probe is None else probe, mode, pooling)
        del keep
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
    mp.fresh_grads(enc)
    return out.detach(), (None if xr.grad is None else xr.grad / gs), grads, list(rt.dropout_state())


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("geo", range(len(GEOMETRIES)))
@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_pixel_gradient_vs_fp64_oracle(cases, mode, geo, pooling):
    """Measured worst error / (limit x max |reference|): DESIGN.md section 4.17."""
    enc, x, ref = cases(geo)
    out64, dx64 = ref[pooling]
    out, dx, grads, _ = run(enc, x, pooling, mode)
    assert dx is not None and dx.shape == x.shape and dx.dtype == torch.float32 and len(grads) > 100
    top = float(dx64.abs().max())
    err = float((dx.double().cpu() - dx64).abs().max())
    e_out = float((out.double().cpu() - out64).abs().max())
    print("\n[pixel gradient %s img%d %s] max |dx| %.3e err %.3e = %.3e of it (limit %.0e, ratio %.3f); output err %.2e"
          % (mode, GEOMETRIES[geo]["img"], pooling, top, err, err / top, TOL[mode], err / (TOL[mode] * top), e_out))
    assert bool(torch.isfinite(dx).all()) and err <= TOL[mode] * top


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_none_pooling_under_the_broadcast_temporal_cotangent_gives_the_temporal_gradient(cases, mode):
    """No extra reference: out_temporal[:, 1 + n] = mean_t out_none[:, t, 1 + n] and out_temporal[:, 0] = out_none[:, t, 0] for every t, so the
    cotangent probe_temporal / T on every frame of 'none' is the cotangent probe_temporal of 'temporal'."""
    enc, x, ref = cases(0)
    B, T, N = x.shape[0], GEOMETRIES[0]["T"], 16
    probe = pool_probe("temporal", (B, 1 + N, 768)).cuda()
    _, dx_t, _, _ = run(enc, x, "temporal", mode)
    _, dx_n, _, _ = run(enc, x, "none", mode, probe=(probe / T).unsqueeze(1).expand(B, T, 1 + N, 768).contiguous())
    top = float(ref["temporal"][1].abs().max())
    err = float((dx_t - dx_n).abs().max())
    print("\n[pixel gradient %s] 'none' under the broadcast cotangent vs 'temporal': err %.3e = %.3e of max %.3e (limit %.0e)" % (mode, err, err / top, top, TOL[mode]))
    assert err <= TOL[mode] * top


@pytest.fixture(scope="module")
def noisy():
    """The img 64 x 3 frames encoder with drop-path 0.2 and attention dropout 0.1 (train mode draws), det_init weights."""
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    from tests.golden.det_init import fill_state_dict_
    from tests.golden.make_golden_pool_modes import pool_clips
    from tests.test_host_cpu import VENC
    geo = GEOMETRIES[0]
    enc = TimeSformer(dict(VENC, num_frm=geo["T"], img_size=geo["img"], drop_path_rate=0.2, attn_drop_rate=0.1), input_format="RGB")
    fill_state_dict_(enc)
    return enc.cuda(), pool_clips(geo).cuda()


def _same(a, b):
    return a.keys() == b.keys() and not [n for n in a if not torch.equal(a[n], b[n])]


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_asking_for_the_pixel_gradient_changes_no_output_gradient_or_draw(noisy, mode):
    """Train mode, drop-path 0.2, attention dropout 0.1, every parameter trainable, the same seeds: outputs, every parameter gradient and the
    dropout-seed counter with x.requires_grad True and False, bit for bit."""
    enc, x = noisy
    enc.train()
    try:
        o0, dx0, g0, s0 = run(enc, x, "temporal", mode, x_grad=False, seed=77)
        o1, dx1, g1, s1 = run(enc, x, "temporal", mode, x_grad=True, seed=77)
        o2, dx2, g2, s2 = run(enc, x, "temporal", mode, x_grad=True, seed=78)
    finally:
        enc.eval()
    assert dx0 is None and dx1 is not None and bool(torch.isfinite(dx1).all()) and float(dx1.abs().max()) > 0
    assert torch.equal(o0, o1) and s0 == s1 and len(g0) > 100
    assert _same(g0, g1), [n for n in g0 if not torch.equal(g0[n], g1[n])][:5]
    assert not torch.equal(o1, o2) and not torch.equal(dx1, dx2), "another seed draws the same masks: train mode did not draw"


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_pixel_gradient_is_bitwise_invariant(cases, mode, pooling):
    """Eval mode, img 48 x 2 frames: x.grad with every parameter frozen (no parameter receives a .grad), under ALPRO_RECOMPUTE, with an
    output_attentions collector and in a second run equals x.grad with every parameter trainable, bit for bit.
    (tests/test_frozen_params_gpu.py holds the data path behind frozen parameters to equality too: torch.equal(dx, dx0).)"""
    enc, x, _ = cases(1)
    o, dx, g, _ = run(enc, x, pooling, mode)
    o2, dx2, g2, _ = run(enc, x, pooling, mode)
    assert torch.equal(o, o2) and torch.equal(dx, dx2) and _same(g, g2), "two runs differ"
    o3, dx3, g3, _ = run(enc, x, pooling, mode, recompute=True)
    assert torch.equal(o, o3) and torch.equal(dx, dx3) and _same(g, g3), "recomputation changes a bit"
    o4, dx4, g4, _ = run(enc, x, pooling, mode, collect=True)
    assert torch.equal(o, o4) and torch.equal(dx, dx4) and _same(g, g4), "a collector changes a bit"
    try:
        for p in enc.parameters():
            p.requires_grad_(False)
        o5, dx5, g5, _ = run(enc, x, pooling, mode)
        o6, dx6, g6, _ = run(enc, x, pooling, mode, recompute=True, collect=True)
    finally:
        for p in enc.parameters():
            p.requires_grad_(True)
    assert g5 == {} and g6 == {}, "a frozen parameter received a .grad"
    assert torch.equal(o, o5) and torch.equal(o, o6)
    assert torch.equal(dx, dx5), "frozen parameters change x.grad: max diff %.3e of %.3e" % (float((dx - dx5).abs().max()), float(dx.abs().max()))
    assert torch.equal(dx, dx6)


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_partially_frozen_encoder_with_an_input_gradient(cases, mode):
    """Blocks 0-5 and the embedding frozen: with an input gradient the prefix is 0 and the backward reaches the pixels (the all-trainable x.grad,
    bit for bit); the trainable blocks' gradients are bitwise those of the run without an input gradient, whose prefix is the 7 frozen stages."""
    from alpro_amd.modeling import train as tr
    enc, x, _ = cases(1)
    m = enc.model
    _, dx_all, g_all, _ = run(enc, x, "temporal", mode)
    frozen = [p for stage in m.stage_params()[:7] for p in stage]
    try:
        for p in frozen:
            p.requires_grad_(False)
        assert tr.frozen_prefix(m.stage_params(), False) == 7 and tr.frozen_prefix(m.stage_params(), True) == 0
        o0, dx0, g0, _ = run(enc, x, "temporal", mode, x_grad=False)
        o1, dx1, g1, _ = run(enc, x, "temporal", mode, x_grad=True)
    finally:
        for p in frozen:
            p.requires_grad_(True)
    names = {n for n, p in enc.named_parameters()}
    want = {n for n in names if n.startswith(("model.norm.",) + tuple("model.blocks.%d." % i for i in range(6, 12)))}
    assert dx0 is None and g0.keys() == g1.keys() == want
    assert torch.equal(dx1, dx_all), "max diff %.3e" % float((dx1 - dx_all).abs().max())
    assert _same(g1, {n: g_all[n] for n in want})
    bad = [n for n in want if not torch.equal(g0[n], g1[n])]
    worst = max((float((g0[n] - g1[n]).abs().max()) / max(float(g1[n].abs().max()), 1e-30) for n in bad), default=0.0)
    print("\n[partially frozen %s] output equal: %s; %d of %d trainable gradients differ between the runs with and without an input gradient, worst %.3e of the tensor's maximum"
          % (mode, torch.equal(o0, o1), len(bad), len(want), worst))
    assert torch.equal(o0, o1) and not bad, bad[:5]


def test_grad_mode_off_gives_the_plain_forward(cases):
    enc, x, _ = cases(1)
    xr = x.clone().requires_grad_(True)
    with torch.no_grad():
        out = enc.forward_features(xr)
        plain = enc.forward_features(x)
    assert not out.requires_grad and out.grad_fn is None and torch.equal(out, plain) and xr.grad is None
    with pytest.raises(AssertionError, match="inference path"):
        enc.forward_cls(xr)


# ------------------------------------------------------------------------------------------------ the full chain
@pytest.fixture(scope="module")
def chain(fixture_models, bert_cfg):
    """The retrieval fixture model (2 frames at 224 px), video 0 against its 3 captions, and the fp64 oracle's d sum_n logits[n, 1] / d video."""
    from oracle import alpro_oracle as ao
    m, batch, _ = fixture_models("retrieval_T2")
    ids, mask, clip = batch["text_input_ids"], batch["text_input_mask"], batch["visual_inputs"][:1].contiguous()
    need = ("visual_encoder.", "text_encoder.bert.", "itm_head.", "vision_proj.", "text_proj.", "temp")
    p = {k: v.detach().double().cpu() for k, v in m.state_dict().items() if k.startswith(need) and not k.startswith("visual_encoder.model.head")}
    v64 = clip.detach().double().cpu().requires_grad_(True)
    with torch.enable_grad():
        out = ao.AlproOracle(p, bert_cfg, 2).forward_inference(dict(visual_inputs=v64, text_input_ids=ids.cpu(), text_input_mask=mask.cpu()))
        out["logits"][:, 1].sum().backward()
    return m, ids, mask, clip, out["logits"].detach(), v64.grad


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_full_chain_pixel_gradient_and_saliency(chain, mode):
    from alpro_amd import config as rt
    from alpro_amd.grounding import pixel_gradient, text_to_pixel_saliency
    m, ids, mask, clip, logits64, dv64 = chain
    n = ids.shape[0]
    clips = clip.expand(n, *clip.shape[1:]).contiguous()      # the pairs (caption b, video 0): their gradients sum to forward_inference's
    frozen = [m.itm_head.bias, m.visual_encoder.model.blocks[3].mlp.fc1.weight]   # a mix of flags to be restored
    for q in frozen:
        q.requires_grad_(False)
    marker = torch.full_like(m.visual_encoder.model.norm.bias, 7.0)
    m.visual_encoder.model.norm.bias.grad = marker.clone()     # a .grad an earlier step left: stays as it is; None stays None
    top = float(dv64.abs().max())
    try:
        flags = [q.requires_grad for q in m.parameters()]
        grads = [q.grad for q in m.parameters()]
        with rt.use_compute_dtype(mode):
            seeds = list(rt.dropout_state())
            g = pixel_gradient(m, ids, mask, clips)
            sal_g = text_to_pixel_saliency(m, ids, mask, clips, method="grad")
            sal_x = text_to_pixel_saliency(m, ids, mask, clips)
            assert list(rt.dropout_state()) == seeds
            assert [q.requires_grad for q in m.parameters()] == flags
            assert all(a is b for a, b in zip(grads, [q.grad for q in m.parameters()]))
            assert torch.equal(m.visual_encoder.model.norm.bias.grad, marker)
            # the same gradient through plain requires_grad_() and forward_inference: one video against the n captions
            for q in m.parameters():
                q.requires_grad_(False)
            v = clip.clone().requires_grad_(True)
            logits = m.forward_inference(dict(visual_inputs=v, text_input_ids=ids, text_input_mask=mask))["logits"]
            scale = 65536.0 if mode == "fp16" else 1.0
            with rt.loss_scaling(object()):
                (logits[:, 1].sum() * scale).backward()
            plain = v.grad / scale
        assert g.shape == clips.shape and g.dtype == torch.float32 and g.is_contiguous() and bool(torch.isfinite(g).all())
        assert v.grad.is_contiguous() and plain.shape == clip.shape
        assert torch.equal(sal_g, g.abs().amax(dim=2)) and torch.equal(sal_x, (g * clips).sum(dim=2)) and sal_g.shape == (n, 2, 224, 224)
        e_sum = float((g.sum(0, keepdim=True).double().cpu() - dv64).abs().max())
        e_plain = float((plain.double().cpu() - dv64).abs().max())
        e_logit = float((logits.detach().double().cpu() - logits64).abs().max())
        print("\n[full chain %s] max |d score / d pixels| %.3e; pixel_gradient summed over the pairs: err %.3e = %.3e of it; plain requires_grad_() through "
              "forward_inference: err %.3e = %.3e of it (limit %.0e); logits err %.2e" % (mode, top, e_sum, e_sum / top, e_plain, e_plain / top, TOL[mode], e_logit))
        assert e_sum <= TOL[mode] * top and e_plain <= TOL[mode] * top
    finally:
        for q, f in zip(m.parameters(), flags):
            q.requires_grad_(f)
        for q in frozen:
            q.requires_grad_(True)
        mp.fresh_grads(m)


def test_helpers_refuse_train_mode(chain):
    from alpro_amd.grounding import pixel_gradient, text_to_pixel_saliency
    m, ids, mask, clip = chain[:4]
    m.train()
    try:
        for fn in (pixel_gradient, text_to_pixel_saliency):
            with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
                fn(m, ids[:1], mask[:1], clip)
    finally:
        m.eval()


# ------------------------------------------------------------------------------------------------ the models' training graphs
@pytest.fixture(scope="module")
def qa2(bert_cfg):
    from tests.test_qa_parity import _qa_batch, _qa_model
    return _qa_model(bert_cfg, 2), _qa_batch(2, 2, "pixel_grad/qa_T2", [1, 0])


CLIP_KEYS = ("visual_inputs", "context_visual_inputs")


def _model_step(m, batch, loss_of, mode, x_grad):
    from alpro_amd import config as rt
    mp.fresh_grads(m)
    rt.seed_dropout(7)
    torch.manual_seed(7)
    np.random.seed(7)     # (AlproForPretrain.forward draws whether the context clips ride along: the same branch in both runs)
    b = dict(batch)
    for k in CLIP_KEYS:
        if k in b:
            b[k] = b[k].detach().clone().requires_grad_(x_grad)
    with rt.use_compute_dtype(mode):
        keep = mp.arm_scale(mode)
        gs = mp.backward(loss_of(m(b)), mode)
        del keep
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    mp.fresh_grads(m)
    return {k: (None if b[k].grad is None else b[k].grad / gs) for k in CLIP_KEYS if k in b}, grads


@pytest.mark.parametrize("which,mode", [("retrieval", "fp32"), ("retrieval", "fp16"), ("pretrain", "fp32"), ("qa", "fp32")])
def test_the_models_deliver_visual_inputs_grad(fixture_models, qa2, monkeypatch, which, mode):
    """AlproForVideoTextRetrieval.forward, AlproForPretrain.forward (visual_inputs and context_visual_inputs as two leaves) and
    AlproForSequenceClassification.forward with requires_grad_() on the clips: visual_inputs receives a finite, non-zero, contiguous gradient of
    its own shape, and no parameter gradient changes a bit against the step without it.  No model detaches or re-wraps the clip.
    context_visual_inputs: the model, like the reference, runs the context clips through the encoder in the same batch (when its draw against
    use_mask_prob says so) and reads none of their output rows, so their gradient is exactly zero when they ride along and None when they do not."""
    monkeypatch.setattr(torch, "multinomial", mp.argmax_multinomial)
    if which == "qa":
        (m, batch), loss_of = qa2, (lambda o: o["loss"])
    elif which == "pretrain":
        (m, batch, _), loss_of = fixture_models("pretrain_release_T4_L30"), (lambda o: o["mlm_loss"] + o["itm_loss"] + o["itc_loss"] + o["mpm_loss"])
    else:
        (m, batch, _), loss_of = fixture_models("retrieval_T2"), (lambda o: o["itm_loss"] + o["itc_loss"])
    none, g0 = _model_step(m, batch, loss_of, mode, False)
    got, g1 = _model_step(m, batch, loss_of, mode, True)
    assert all(v is None for v in none.values()) and len(g0) > 100
    for k, v in got.items():
        if k == "context_visual_inputs":
            assert v is None or (v.shape == batch[k].shape and not bool(v.any())), "the context clips' output rows are read by nobody"
            continue
        assert v is not None and v.shape == batch[k].shape and v.dtype == torch.float32 and v.is_contiguous(), k
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
        print("\n[%s %s] max |d loss / d %s| %.3e" % (which, mode, k, float(v.abs().max())))
    assert (which == "pretrain") == ("context_visual_inputs" in got)
    assert _same(g0, g1), [n for n in g0 if n not in g1 or not torch.equal(g0[n], g1[n])][:5]
