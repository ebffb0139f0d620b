"""GPU: the Grad-CAM path on the 2 text + 2 fusion layer model of tests/test_attn_probs_gpu.py (D = 768, L = 22): BertModel.forward(attn_grads=)
changes no output, gradient or dropout draw; the frozen prefix is shortened for a chosen layer; the refusals; every collected G against a torch
fp64 autograd restatement of the pass (retain_grad() on each softmax); the reference-style getters; grounding.text_to_patch_gradcam.

Limits, as a fraction of a map's maximum: fp32 the project's exact-mode 2e-4 (the attention-map tests), fp16 the 1e-2 that
tests/test_model_parity.py applies to fp16 gradients against the reference (test_pretrain_gradients_vs_reference)."""
import math

import numpy as np
import pytest
import torch

from tests.conftest import BERT_CFG
from tests.test_attn_probs_gpu import B, D, LT, LV, NH, QK_GAIN, _Pair
from tests.test_host_cpu import make_cfg

pytestmark = pytest.mark.gpu

L = LT + LV
TOL = {"fp32": 2e-4, "fp16": 1e-2}
SCALE = {"fp32": 1.0, "fp16": 4096.0}     # fp16 operands need a scaled backward; the scale tests/test_model_parity.py uses


@pytest.fixture(scope="module")
def model():
    """The model of tests/test_attn_probs_gpu.py, with attention-probability dropout off (hidden dropout stays at 0.1: train mode still draws)."""
    from alpro_amd.modeling.xbert import BertModel
    from tests.golden.det_init import det_param, fill_state_dict_, unit_uniform
    cfg = make_cfg(dict(BERT_CFG, num_hidden_layers=4, fusion_layer=2, vocab_size=2048, attention_probs_dropout_prob=0.0))
    m = fill_state_dict_(BertModel(cfg, add_pooling_layer=False))
    with torch.no_grad():
        for layer in m.encoder.layer:
            for lin in (layer.attention.self.query, layer.attention.self.key):
                lin.weight.mul_(QK_GAIN)
                lin.bias.mul_(QK_GAIN)
    m = m.eval().cuda()
    x = (unit_uniform("attn_model/ids", B * LT) + 1.0) * 0.5
    ids = torch.from_numpy((110 + np.floor(x * 1900)).astype(np.int64).reshape(B, LT))
    ids[:, 0] = 101
    mask = torch.ones(B, LT, dtype=torch.long)
    mask[1, LT - 3:] = 0
    ids[1, LT - 3:] = 0
    emb = torch.from_numpy((1.5 * unit_uniform("attn_model/embeds", B * L * D)).astype(np.float32).reshape(B, L, D))
    att = torch.cat([mask, torch.ones(B, LV, dtype=torch.long)], dim=1)
    w = torch.from_numpy(unit_uniform("gradcam/score_weight", B * L * D).astype(np.float32).reshape(B, L, D))
    head = torch.nn.Linear(D, 2)
    with torch.no_grad():
        head.weight.copy_(det_param("gradcam/itm_head.weight", (2, D)))
        head.bias.copy_(det_param("gradcam/itm_head.bias", (2,)))
    return m, ids.cuda(), mask.cuda(), emb.cuda(), att.cuda(), w.cuda(), head.cuda()


class PairITM(_Pair):
    """_Pair plus the ITM head: what text_to_patch_gradcam reads of an AlproBaseModel."""

    def __init__(self, bert, head):
        super().__init__(bert)
        self.itm_head = head


def scaled_backward(score, dtype):
    """score.backward() the way the operand dtype needs it (fp16: scaled, inside rt.loss_scaling); returns the factor the gradients carry."""
    from alpro_amd import config as rt
    s = SCALE[dtype]
    if s == 1.0:
        score.backward()
    else:
        with rt.loss_scaling(object()):
            (score * s).backward()
    return s


def _clear(m):
    for p in m.parameters():
        p.grad = None


def _pass_inputs(model, mode, variant):
    m, ids, mask, emb, att, w, _ = model
    if mode == "text":
        return dict(attention_mask=mask, mode="text"), [emb[:, :LT].contiguous()], w[:, :LT]
    if variant == "out_rows":
        rows = torch.tensor([0, 5, L, L + LT], device="cuda")
        return dict(attention_mask=att, mode="fusion", out_rows=rows), [emb], w.reshape(B * L, D)[:4]
    if variant == "parts":
        ti, vi = torch.tensor([1, 0, 1], device="cuda"), torch.tensor([0, 0, 1], device="cuda")
        att3 = torch.cat([att[ti, :LT], att[vi, LT:]], dim=1)
        return (dict(attention_mask=att3, mode="fusion", parts_index=(ti, vi)), [emb[:, :LT].contiguous(), emb[:, LT:].contiguous()],
                torch.cat([w, w[:1]], dim=0))
    return dict(attention_mask=att, mode="fusion"), [emb], w


@pytest.mark.parametrize("dtype", ("fp32", "fp16"))
@pytest.mark.parametrize("mode,variant", [("fusion", "plain"), ("text", "plain"), ("fusion", "out_rows"), ("fusion", "parts")])
def test_a_collector_changes_no_output_gradient_or_dropout_draw(model, mode, variant, dtype):
    """Train mode (hidden dropout draws), every parameter trainable: the pass with and without attn_grads from the same dropout seed."""
    from alpro_amd import config as rt
    from alpro_amd.modeling.xbert import AttnGradients
    m = model[0]
    kw, acts, w = _pass_inputs(model, mode, variant)
    kw = dict(kw)
    pidx = kw.pop("parts_index", None)
    lo, hi = m.encoder.layer_range(mode)
    params = [p for i in range(lo, hi) for p in m.encoder.layer[i].parameters()]
    m.train()
    try:
        res = []
        for col in (None, AttnGradients(want=("grad", "cam"), grad_scale=SCALE[dtype])):
            _clear(m)
            rt.seed_dropout(20240611)
            xs = [a.clone().requires_grad_(True) for a in acts]
            with rt.use_compute_dtype(dtype):
                if pidx is not None:
                    o = m(encoder_embeds_parts=(xs[0], xs[1], pidx[0], pidx[1]), attn_grads=col, **kw)
                else:
                    o = m(encoder_embeds=xs[0], attn_grads=col, **kw)
                scaled_backward((o.last_hidden_state * w).sum(), dtype)
            torch.cuda.synchronize()
            res.append((o.last_hidden_state.detach().clone(), [x.grad.clone() for x in xs], [p.grad.clone() for p in params], list(rt.dropout_state()), col))
    finally:
        m.eval()
        _clear(m)
    (o0, dx0, g0, seed0, _), (o1, dx1, g1, seed1, col) = res
    assert torch.equal(o0, o1) and seed0 == seed1
    assert len(dx0) == len(dx1) and all(torch.equal(a, b) for a, b in zip(dx0, dx1))
    assert len(g0) == len(g1) > 0 and all(torch.equal(a, b) for a, b in zip(g0, g1))
    nb = o0.shape[0] if variant != "out_rows" else B
    Lm = LT if mode == "text" else L
    assert sorted(col.grads) == sorted(col.cams) == list(range(hi - lo))
    for i in range(hi - lo):
        assert col.grads[i].shape == col.cams[i].shape == (nb, NH, Lm, Lm) and col.grads[i].dtype == torch.float32
        assert bool(torch.isfinite(col.grads[i]).all()) and float(col.grads[i].abs().max()) > 0 and float(col.cams[i].min()) >= 0


def test_a_frozen_prefix_is_shortened_for_a_chosen_layer_and_unchanged_without_a_collector(model):
    from alpro_amd import config as rt
    from alpro_amd.modeling.xbert import AttnGradients
    m, _, _, emb, att, w, _ = model
    first, last = m.encoder.layer[2], m.encoder.layer[3]
    frozen = list(m.embeddings.parameters()) + list(first.parameters())

    def run(col, freeze):
        _clear(m)
        for p in frozen:
            p.requires_grad_(not freeze)
        try:
            with rt.use_compute_dtype("fp32"):
                o = m(encoder_embeds=emb, attention_mask=att, mode="fusion", attn_grads=col)     # (emb needs no gradient)
                (o.last_hidden_state * w).sum().backward()
            torch.cuda.synchronize()
            return (o.last_hidden_state.detach().clone(), [None if p.grad is None else p.grad.clone() for p in first.parameters()],
                    [p.grad.clone() for p in last.parameters()])
        finally:
            for p in frozen:
                p.requires_grad_(True)
            _clear(m)

    all_col, fr_col = AttnGradients(layers=(0,), want=("grad",)), AttnGradients(layers=(0,), want=("grad",))
    o_all, g_first_all, g_last_all = run(all_col, freeze=False)
    o_plain, g_first_plain, g_last_plain = run(None, freeze=True)
    o_col, g_first_col, g_last_col = run(fr_col, freeze=True)
    assert all(g is not None for g in g_first_all)
    assert all(g is None for g in g_first_plain) and all(g is None for g in g_first_col)          # frozen stays frozen, collector or not
    assert torch.equal(o_all, o_plain) and torch.equal(o_plain, o_col)
    assert all(torch.equal(a, b) for a, b in zip(g_last_plain, g_last_col)) and all(torch.equal(a, b) for a, b in zip(g_last_all, g_last_col))
    assert float(fr_col.grads[0].abs().max()) > 0 and torch.equal(fr_col.grads[0], all_col.grads[0])   # the map of the frozen layer, same bits


def test_refusals(model):
    from alpro_amd import config as rt
    from alpro_amd.modeling.xbert import AttnGradients
    m, _, _, emb, att, w, _ = model
    x = emb.clone().requires_grad_(True)
    with rt.use_compute_dtype("fp32"):
        with torch.no_grad(), pytest.raises(RuntimeError, match="grad mode is off"):
            m(encoder_embeds=x, attention_mask=att, mode="fusion", attn_grads=AttnGradients())
        for p in m.parameters():
            p.requires_grad_(False)
        try:
            with pytest.raises(RuntimeError, match="nothing to differentiate"):
                m(encoder_embeds=emb, attention_mask=att, mode="fusion", attn_grads=AttnGradients())
            col = AttnGradients(want=("grad", "cam"))
            o = m(encoder_embeds=x, attention_mask=att, mode="fusion", attn_grads=col)            # an input alone is enough
            with pytest.raises(RuntimeError, match=r"backward\(\) has not run"):
                col.grads
            (o.last_hidden_state * w).sum().backward()
            assert len(col.grads) == len(col.cams) == 2 and all(p.grad is None for p in m.parameters())
        finally:
            for p in m.parameters():
                p.requires_grad_(True)
        m.config.attention_probs_dropout_prob = 0.1
        m.train()
        try:
            with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
                m(encoder_embeds=x, attention_mask=att, mode="fusion", attn_grads=AttnGradients())
            m(encoder_embeds=x, attention_mask=att, mode="fusion")                                # without a collector: as before
        finally:
            m.config.attention_probs_dropout_prob = 0.0
            m.eval()
            _clear(m)


# ---- the fp64 autograd restatement ------------------------------------------------------------------------------------------------------------
def _lin64(x, lin):
    return x @ lin.weight.detach().double().cpu().t() + lin.bias.detach().double().cpu()


def _ln64(x, ln, eps):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), ln.weight.detach().double().cpu(), ln.bias.detach().double().cpu(), eps)


def restate64(m, mode, x, key_bias):
    """x (B, L, D) fp64 leaf or not, on the CPU -> (output (B, L, D), [softmax of every layer, each with retain_grad()])."""
    lo, hi = m.encoder.layer_range(mode)
    h, probs = x, []
    eps = m.config.layer_norm_eps
    kb = key_bias.detach().double().cpu()[:, None, None, :]
    for i in range(lo, hi):
        layer = m.encoder.layer[i]
        sa, so = layer.attention.self, layer.attention.output
        nb, nl = h.shape[0], h.shape[1]
        q, k, v = (_lin64(h, lin).view(nb, nl, NH, 64).transpose(1, 2) for lin in (sa.query, sa.key, sa.value))
        p = (q @ k.transpose(-1, -2) / 8.0 + kb).softmax(-1)
        p.retain_grad()
        probs.append(p)
        ctx = (p @ v).transpose(1, 2).reshape(nb, nl, -1)
        a = _ln64(h + _lin64(ctx, so.dense), so.LayerNorm, eps)
        u = _lin64(a, layer.intermediate.dense)
        it = 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
        h = _ln64(a + _lin64(it, layer.output.dense), layer.output.LayerNorm, eps)
    return h, probs


@pytest.mark.parametrize("dtype", ("fp32", "fp16"))
@pytest.mark.parametrize("mode", ("fusion", "text"))
def test_collected_gradients_match_the_fp64_autograd_restatement(model, mode, dtype):
    from alpro_amd import config as rt
    from alpro_amd.modeling.xbert import AttnGradients
    m, _, mask, emb, att, w, _ = model
    x0, am, wm = (emb, att, w) if mode == "fusion" else (emb[:, :LT].contiguous(), mask, w[:, :LT])
    col = AttnGradients(want=("grad", "cam"), grad_scale=SCALE[dtype])
    x = x0.clone().requires_grad_(True)
    with rt.use_compute_dtype(dtype):
        o = m(encoder_embeds=x, attention_mask=am, mode=mode, attn_grads=col, output_attentions=True)
        scaled_backward((o.last_hidden_state * wm).sum(), dtype)
    _clear(m)
    out64, probs = restate64(m, mode, x0.double().cpu().requires_grad_(True), m.key_bias(am))
    (out64 * wm.double().cpu()).sum().backward()
    for i, p in enumerate(probs):
        ref = p.grad.numpy()
        got = col.grads[i].cpu().numpy().astype(np.float64)
        err, top = np.abs(got - ref).max(), np.abs(ref).max()
        cam_ref = p.detach().numpy() * np.maximum(ref, 0.0)
        cerr, ctop = np.abs(col.cams[i].cpu().numpy().astype(np.float64) - cam_ref).max(), cam_ref.max()
        print("[gradcam] %s %s layer %d: G max err %.3e = %.3e of max |G| %.3e; CAM max err %.3e = %.3e of max %.3e (limit %.0e)"
              % (mode, dtype, i, err, err / top, top, cerr, cerr / ctop, ctop, TOL[dtype]))
        assert err <= TOL[dtype] * top and cerr <= TOL[dtype] * ctop
        assert torch.equal(col.cams[i], o.attentions[i] * col.grads[i].clamp(min=0))      # P is the `attentions` entry, bit for bit


def test_getters_equal_the_full_window_collector(model):
    from alpro_amd import config as rt
    from alpro_amd.modeling.xbert import AttnGradients
    m, _, _, emb, att, w, _ = model
    sa = [m.encoder.layer[i].attention.self for i in (2, 3)]
    assert all(s.save_attention is False and s.get_attention_map() is None and s.get_attn_gradients() is None for s in sa)
    col = AttnGradients(want=("grad",))
    x = emb.clone().requires_grad_(True)
    sa[1].save_attention = True
    try:
        with rt.use_compute_dtype("fp32"):
            o = m(encoder_embeds=x, attention_mask=att, mode="fusion", attn_grads=col, output_attentions=True)
            (o.last_hidden_state * w).sum().backward()
    finally:
        sa[1].save_attention = False
        _clear(m)
    assert sa[0].get_attention_map() is None and sa[0].get_attn_gradients() is None          # the flag is per layer
    assert torch.equal(sa[1].get_attention_map(), o.attentions[1]) and torch.equal(sa[1].get_attn_gradients(), col.grads[1])
    sa[1].attention_map = sa[1].attn_gradients = None


def _manual_gradcam(pair, ids, mask, video, layers, dtype, scale):
    """What text_to_patch_gradcam does, spelled out with the public pieces."""
    from alpro_amd import config as rt
    from alpro_amd.modeling.alpro_models import _linear32
    from alpro_amd.modeling.xbert import AttnGradients
    bert = pair.text_encoder
    Lv = video.shape[1]
    col = AttnGradients(layers=layers, window=((0, LT), (LT + 1, LT + Lv)), want=("cam",), grad_scale=scale)
    with torch.no_grad():
        te = pair._text_embeds(ids, mask)
    v = video.detach().clone().requires_grad_(True)
    att = torch.cat([mask, torch.ones(B, Lv, dtype=mask.dtype, device="cuda")], dim=1)
    flags = [(p, p.requires_grad) for p in pair.parameters()]
    for p, _ in flags:
        p.requires_grad_(False)
    try:
        out = bert(encoder_embeds=torch.cat([te, v], dim=1), attention_mask=att, mode="fusion", attn_grads=col).last_hidden_state
        score = _linear32(out[:, 0, :], pair.itm_head)[:, 1].sum() * scale
        with rt.loss_scaling(object()):
            score.backward()
    finally:
        for p, f in flags:
            p.requires_grad_(f)
    acc = None
    n = len(bert.encoder.layer) - bert.config.fusion_layer
    for i in layers:
        c = col.cams[i % n].mean(dim=1)
        acc = c if acc is None else acc + c
    hg = math.isqrt(Lv - 1)
    return (acc / float(len(layers))).view(B, LT, hg, hg)


@pytest.mark.parametrize("layers", ((-1,), (0, 1)))
def test_text_to_patch_gradcam_is_the_mean_of_the_windowed_cams_and_leaves_the_model_untouched(model, layers):
    from alpro_amd import config as rt
    from alpro_amd.grounding import text_to_patch_gradcam
    m, ids, mask, emb, _, _, head = model
    video = emb[:, LT:].contiguous()
    pair = PairITM(m, head).eval()
    frozen = [m.encoder.layer[0].output.dense.weight, head.bias]       # a mix of flags to be restored
    for p in frozen:
        p.requires_grad_(False)
    marker = torch.full_like(m.encoder.layer[3].output.dense.bias, 7.0)
    m.encoder.layer[3].output.dense.bias.grad = marker.clone()         # a .grad an earlier step left: stays as it is; None stays None
    try:
        flags = [p.requires_grad for p in pair.parameters()]
        grads = [p.grad for p in pair.parameters()]
        maps = {}
        for dtype in ("fp32", "fp16"):
            with rt.use_compute_dtype(dtype):
                seeds = list(rt.dropout_state())
                got = text_to_patch_gradcam(pair, ids, mask, video, layers=layers)
                assert list(rt.dropout_state()) == seeds
                assert [p.requires_grad for p in pair.parameters()] == flags
                assert all(a is b for a, b in zip(grads, [p.grad for p in pair.parameters()]))
                assert torch.equal(m.encoder.layer[3].output.dense.bias.grad, marker)
                want = _manual_gradcam(pair, ids, mask, video, layers, dtype, 65536.0 if dtype == "fp16" else 1.0)
            hg = math.isqrt(LV - 1)
            assert got.shape == (B, LT, hg, hg) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
            assert torch.equal(got, want) and float(got.max()) > 0 and float(got.min()) >= 0
            maps[dtype] = got
        err, top = float((maps["fp16"] - maps["fp32"]).abs().max()), float(maps["fp32"].max())
        print("[gradcam] text_to_patch_gradcam layers=%s: fp16 (default grad_scale 2^16) vs fp32 max err %.3e = %.3e of max %.3e (limit %.0e)"
              % (layers, err, err / top, top, TOL["fp16"]))
        assert err <= TOL["fp16"] * top
    finally:
        for p in frozen:
            p.requires_grad_(True)
        _clear(m)
        head.weight.grad = head.bias.grad = None
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
        text_to_patch_gradcam(pair.train(), ids, mask, video)
    pair.eval()
    with pytest.raises(ValueError, match="outside the 2 fusion layers"):
        text_to_patch_gradcam(pair, ids, mask, video, layers=(2,))
