"""GPU: alpro_attn_probs against the fp64 softmax inside the bound derived in tests/attn_probs_cases.py (computed from each case's inputs and
the observed error of the forward kernel's log-sum-exp rows; no tuned constant), its window / reproducibility properties, and the
output_attentions / output_hidden_states plumbing of BertModel with the grounding helper on top (2 text + 2 fusion layers at D = 768)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import attn_probs_cases as ac
from tests.conftest import BERT_CFG
from tests.test_host_cpu import make_cfg

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(L, dtype, H=2, bias="mixed", peaked=False):
    return ac.peaked_case(L, dtype) if peaked else ac.random_case(L, dtype, H=H, bias=bias)


def _dev(case):
    qkv = torch.from_numpy(case.qkv).cuda().to(ac.TORCH_DTYPE[case.dtype])
    kb = None if case.bias is None else torch.from_numpy(case.bias).cuda()
    return qkv, kb


def _run(case, q_range=None, k_range=None):
    """-> (probabilities, lse, attention output) on the device: lse from the forward kernel, as in the model."""
    from alpro_amd import hip
    qkv, kb = _dev(case)
    out, lse = hip.attn(qkv, case.batch, case.L, case.H, case.scale, kb, want_lse=True)
    p = hip.attn_probs(qkv, lse, case.batch, case.L, case.H, case.scale, kb, q_range=q_range, k_range=k_range)
    return p, lse, out


@pytest.mark.parametrize("dtype", ac.DTYPES)
@pytest.mark.parametrize("L", ac.LENGTHS)
def test_probabilities_inside_the_bound(L, dtype):
    c = _case(L, dtype)
    p, lse, _ = _run(c)
    assert p.shape == (c.batch, c.H, L, L) and p.dtype == torch.float32 and p.is_contiguous()
    ac.check(c, p.cpu().numpy(), lse.cpu().numpy())


@pytest.mark.parametrize("L,dtype,H,bias", [(65, "fp16", 12, "mixed"), (65, "fp32", 2, "none"), (300, "bf16", 2, "none")])
def test_probabilities_inside_the_bound_twelve_heads_and_no_bias(L, dtype, H, bias):
    c = _case(L, dtype, H=H, bias=bias)
    p, lse, _ = _run(c)
    ac.check(c, p.cpu().numpy(), lse.cpu().numpy())


@pytest.mark.parametrize("dtype", ac.DTYPES)
@pytest.mark.parametrize("L", (65, 300))
def test_peaked_scores_stay_finite_and_below_one(L, dtype):
    c = _case(L, dtype, peaked=True)
    p, lse, _ = _run(c)
    pn = p.cpu().numpy()
    assert np.isfinite(pn).all() and pn.max() <= 1.0 and pn.min() >= 0.0
    ac.check(c, pn, lse.cpu().numpy())


WINDOWS = (((5, 45), (33, 103)),        # q0 / k0 no multiples of 32, nk no multiple of 4
           ((37, 38), (0, None)),       # nq = 1
           ((0, None), (70, 71)),       # nk = 1
           ((3, 67), (41, 105)),        # nk = 64: full tiles at an unaligned k0 (the 16-byte store path)
           ((200, None), (129, None)),  # ends at L on both sides
           ((31, 33), (31, 33)))        # two rows / keys across a tile edge


@pytest.mark.parametrize("dtype", ("fp32", "fp16"))
@pytest.mark.parametrize("L", (237, 300))
def test_a_window_is_the_same_slice_of_the_full_map_bit_for_bit(L, dtype):
    c = _case(L, dtype)
    full, _, _ = _run(c)
    for (qa, qb), (ka, kb) in WINDOWS:
        qb, kb = L if qb is None else qb, L if kb is None else kb
        w, _, _ = _run(c, q_range=(qa, qb), k_range=(ka, kb))
        assert w.shape == (c.batch, c.H, qb - qa, kb - ka) and w.is_contiguous()
        assert torch.equal(w, full[:, :, qa:qb, ka:kb]), ((qa, qb), (ka, kb))


@pytest.mark.parametrize("L,dtype", [(300, "bf16"), (65, "fp32")])
def test_two_runs_are_bitwise_equal(L, dtype):
    c = _case(L, dtype)
    a, _, _ = _run(c)
    b, _, _ = _run(c)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-4), ("fp16", 8e-4)])
@pytest.mark.parametrize("L", (65, 300))
def test_probabilities_times_values_give_the_attention_output(L, dtype, tol):
    # (bias 'pad': trailing and middle keys masked, no all-masked sequence -- there every score sits at -10000, fp32 resolves it to 2^-10 and the
    # two kernels round it in different units (natural log / log2): a relative 1e-3 on P that is the bound test's business, not this one's)
    c = _case(L, dtype, bias="pad")
    p, _, out = _run(c)
    ref = out.float().cpu().numpy().astype(np.float64).reshape(c.batch, L, c.H, 64).transpose(0, 2, 1, 3)     # hip.attn's output, (batch, H, L, 64)
    got = p.cpu().numpy().astype(np.float64) @ ac.values64(c.qkv, c.batch, L, c.H)
    err, lim = np.abs(got - ref).max(), tol * np.abs(ref).max()
    print("P @ V vs hip.attn (L=%d %s): max err %.3e, limit %.3e" % (L, dtype, err, lim))
    assert err <= lim


def test_wrapper_refuses_shapes_and_windows_it_cannot_take():
    from alpro_amd import hip
    c = _case(33, "fp16")
    qkv, kb = _dev(c)
    lse = torch.zeros(c.batch, c.H, c.L, device="cuda")
    for kw, msg in ((dict(q_range=(0, 34)), "q0=0 nq=34"), (dict(k_range=(5, 5)), "nk=0"), (dict(k_range=(-1, 4)), "k0=-1"), (dict(q_range=(9, 3)), "nq=-6")):
        with pytest.raises(RuntimeError, match=msg):
            hip.attn_probs(qkv, lse, c.batch, c.L, c.H, c.scale, kb, **kw)
    with pytest.raises(RuntimeError, match="lse must be"):
        hip.attn_probs(qkv, lse[:, :1], c.batch, c.L, c.H, c.scale, kb)
    with pytest.raises(RuntimeError, match="qkv must be"):
        hip.attn_probs(qkv[:, :128], lse, c.batch, c.L, c.H, c.scale, kb)
    with pytest.raises(RuntimeError, match="key_bias must be"):
        hip.attn_probs(qkv, lse, c.batch, c.L, c.H, c.scale, kb[:, :4])


# ---- the model: 2 text + 2 fusion layers at D = 768 ------------------------------------------------------------------------------------------
B, LT, LV, D, NH = 2, 12, 10, 768, 12      # 12 caption tokens (the second caption padded) + a video [CLS] and a 3 x 3 patch grid: L = 22
QK_GAIN = 2.0                              # scores with a standard deviation of about 1 instead of a quarter: peaked maps


@pytest.fixture(scope="module")
def model():
    from alpro_amd.modeling.xbert import BertModel
    from tests.golden.det_init import fill_state_dict_, unit_uniform
    m = fill_state_dict_(BertModel(make_cfg(dict(BERT_CFG, num_hidden_layers=4, fusion_layer=2, vocab_size=2048)), add_pooling_layer=False))
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
    emb = torch.from_numpy((1.5 * unit_uniform("attn_model/embeds", B * (LT + LV) * D)).astype(np.float32).reshape(B, LT + LV, D))
    att = torch.cat([mask, torch.ones(B, LV, dtype=torch.long)], dim=1)
    return m, ids.cuda(), mask.cuda(), emb.cuda(), att.cuda()


def _inputs(model, mode):
    m, ids, mask, emb, att = model
    if mode == "fusion":
        return dict(encoder_embeds=emb, attention_mask=att, mode=mode), LT + LV, 2
    return dict(input_ids=ids, attention_mask=mask, mode=mode), LT, (2 if mode == "text" else 4)


def _layer_probs64(layer, h, key_bias, dtype):
    """fp64 restatement of one layer's softmax from its input hidden state (B, L, D): operands rounded to the operand dtype where the kernels
    round them (the layer input, the weights, the stored q | k), everything else in fp64."""
    sa = layer.attention.self
    x = ac.round_to(h.float().cpu().numpy(), dtype).astype(np.float64)
    qk = []
    for lin in (sa.query, sa.key):
        w = ac.round_to(lin.weight.detach().float().cpu().numpy(), dtype).astype(np.float64)
        y = x @ w.T + lin.bias.detach().float().cpu().numpy().astype(np.float64)
        qk.append(ac.round_to(y.astype(np.float32), dtype).astype(np.float64).reshape(h.shape[0], h.shape[1], NH, 64).transpose(0, 2, 1, 3))
    s = qk[0] @ qk[1].transpose(0, 1, 3, 2) / 8.0 + key_bias.float().cpu().numpy().astype(np.float64)[:, None, None, :]
    s = s - s.max(axis=-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(axis=-1, keepdims=True)


@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-4), ("fp16", 8e-4)])
@pytest.mark.parametrize("mode", ("text", "fusion", "multi_modal"))
def test_model_outputs_have_the_right_shapes_change_nothing_and_match_fp64(model, mode, dtype, tol):
    from alpro_amd import config as rt
    m = model[0]
    kw, L, n = _inputs(model, mode)
    lo, hi = m.encoder.layer_range(mode)
    assert hi - lo == n
    with rt.use_compute_dtype(dtype), torch.no_grad():
        plain = m(return_dict=True, **kw)
        both = m(return_dict=True, output_attentions=True, output_hidden_states=True, **kw)
        only_att = m(return_dict=True, output_attentions=True, **kw)
        tup = m(return_dict=False, output_attentions=True, output_hidden_states=True, **kw)
    assert plain.attentions is None and plain.hidden_states is None
    assert both.attentions is not None and both.hidden_states is not None
    assert only_att.hidden_states is None and len(only_att.attentions) == n
    assert torch.equal(plain.last_hidden_state, both.last_hidden_state) and torch.equal(plain.last_hidden_state, only_att.last_hidden_state)
    assert isinstance(both.attentions, tuple) and isinstance(both.hidden_states, tuple) and len(both.attentions) == n and len(both.hidden_states) == n + 1
    assert len(tup) == 4 and tup[1] is None and torch.equal(tup[0], plain.last_hidden_state)            # (sequence, pooled, hidden_states, attentions)
    assert len(tup[2]) == n + 1 and len(tup[3]) == n and torch.equal(tup[3][0], both.attentions[0])
    for h in both.hidden_states:
        assert h.shape == (B, L, D) and h.dtype == torch.float32 and not h.requires_grad
    assert torch.equal(both.hidden_states[-1], both.last_hidden_state) and both.hidden_states[-1].data_ptr() != both.last_hidden_state.data_ptr()
    kb = m.key_bias(kw["attention_mask"])
    for i, a in enumerate(both.attentions):
        assert a.shape == (B, NH, L, L) and a.dtype == torch.float32 and not a.requires_grad
        assert torch.equal(a, only_att.attentions[i])
        ref = _layer_probs64(m.encoder.layer[lo + i], both.hidden_states[i], kb, dtype)
        err = np.abs(a.cpu().numpy().astype(np.float64) - ref).max()
        print("%s %s attentions[%d] vs fp64 restatement: max err %.3e (limit %.1e of max %.3f)" % (mode, dtype, i, err, tol, ref.max()))
        assert err <= tol * ref.max()


@pytest.mark.parametrize("dtype", ("fp32", "fp16"))
def test_model_outputs_with_out_rows_and_with_the_config_flags(model, dtype):
    from alpro_amd import config as rt
    m, _, _, emb, att = model
    L = LT + LV
    rows = torch.tensor([0, 5, L, L + LT], device="cuda")
    with rt.use_compute_dtype(dtype), torch.no_grad():
        plain = m(encoder_embeds=emb, attention_mask=att, mode="fusion", out_rows=rows)
        full = m(encoder_embeds=emb, attention_mask=att, mode="fusion", output_attentions=True, output_hidden_states=True)
        m.config.output_attentions, m.config.output_hidden_states = True, True      # the flags default from the config (xbert.py:977-980)
        try:
            sub = m(encoder_embeds=emb, attention_mask=att, mode="fusion", out_rows=rows)
            off = m(encoder_embeds=emb, attention_mask=att, mode="fusion", out_rows=rows, output_attentions=False, output_hidden_states=False)
        finally:
            del m.config.output_attentions, m.config.output_hidden_states
    assert off.attentions is None and off.hidden_states is None
    assert torch.equal(plain.last_hidden_state, sub.last_hidden_state) and sub.last_hidden_state.shape == (4, D)
    assert len(sub.attentions) == 2 and len(sub.hidden_states) == 3
    assert sub.hidden_states[-1].shape == (4, D) and torch.equal(sub.hidden_states[-1], sub.last_hidden_state)
    for i in range(2):
        assert sub.hidden_states[i].shape == (B, L, D) and torch.equal(sub.hidden_states[i], full.hidden_states[i])
        assert sub.attentions[i].shape == (B, NH, L, L) and torch.equal(sub.attentions[i], full.attentions[i])
    assert torch.equal(sub.hidden_states[0], emb) and sub.hidden_states[0].data_ptr() != emb.data_ptr()      # a copy, not the caller's tensor


def test_model_outputs_with_encoder_embeds_parts(model):
    from alpro_amd import config as rt
    m, _, _, emb, att = model
    text_pool, video_pool = emb[:, :LT].contiguous(), emb[:, LT:].contiguous()
    ti, vi = torch.tensor([1, 0, 1], device="cuda"), torch.tensor([0, 0, 1], device="cuda")
    att3 = torch.cat([att[ti, :LT], att[vi, LT:]], dim=1)
    with rt.use_compute_dtype("fp16"), torch.no_grad():
        cat = m(encoder_embeds=torch.cat([text_pool[ti], video_pool[vi]], dim=1), attention_mask=att3, mode="fusion", output_attentions=True, output_hidden_states=True)
        got = m(encoder_embeds_parts=(text_pool, video_pool, ti, vi), attention_mask=att3, mode="fusion", output_attentions=True, output_hidden_states=True)
    assert torch.equal(cat.last_hidden_state, got.last_hidden_state)
    assert len(got.attentions) == 2 and len(got.hidden_states) == 3
    for a, b in zip(cat.attentions + cat.hidden_states, got.attentions + got.hidden_states):
        assert a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("mode", ("text", "fusion"))
def test_anchored_path_returns_the_outputs_and_keeps_every_gradient_bit(model, mode):
    """Train mode, bf16 operands, dropout on: the anchored (_BertRun) pass with and without the two flags, from the same dropout seed."""
    from alpro_amd import config as rt
    m = model[0]
    _, _, mask, emb, att = model
    lo, hi = m.encoder.layer_range(mode)
    L = LT + LV if mode == "fusion" else LT
    x0 = emb if mode == "fusion" else emb[:, :LT].contiguous()
    am = att if mode == "fusion" else mask
    params = [p for i in range(lo, hi) for p in m.encoder.layer[i].parameters()]
    m.train()
    try:
        res = []
        for flags in (False, True):
            for p in m.parameters():
                p.grad = None
            rt.seed_dropout(20240607)
            x = x0.clone().requires_grad_(True)
            with rt.use_compute_dtype("bf16"):
                o = m(encoder_embeds=x, attention_mask=am, mode=mode, output_attentions=flags, output_hidden_states=flags)
                assert o.last_hidden_state.requires_grad
                (o.last_hidden_state * torch.linspace(-1, 1, D, device="cuda")).sum().backward()
            torch.cuda.synchronize()
            res.append((o, x.grad.clone(), [p.grad.clone() for p in params], rt.next_dropout_seed()))
    finally:
        m.eval()
        for p in m.parameters():
            p.grad = None
    (o0, dx0, g0, seed0), (o1, dx1, g1, seed1) = res
    assert o0.attentions is None and o0.hidden_states is None
    assert torch.equal(o0.last_hidden_state, o1.last_hidden_state) and torch.equal(dx0, dx1) and seed0 == seed1
    assert len(g0) == len(g1) > 0 and all(torch.equal(a, b) for a, b in zip(g0, g1))
    assert len(o1.attentions) == hi - lo and len(o1.hidden_states) == hi - lo + 1
    kb = m.key_bias(am)
    for i, a in enumerate(o1.attentions):
        assert a.shape == (B, NH, L, L) and not a.requires_grad and a.grad_fn is None
        # the probabilities BEFORE dropout: rows sum to 1 (a map with a tenth of its entries dropped and the rest scaled by 1 / 0.9 does not) and
        # match the fp64 restatement of the layer on the returned hidden state at bf16's parity tolerance (6e-3, tests/test_model_parity.py)
        assert float((a.sum(-1) - 1).abs().max()) < 1e-5 and float((a == 0).float().mean()) < 0.2
        ref = _layer_probs64(m.encoder.layer[lo + i], o1.hidden_states[i], kb, "bf16")
        assert np.abs(a.cpu().numpy().astype(np.float64) - ref).max() <= 6e-3 * ref.max()
    for h in o1.hidden_states:
        assert h.shape == (B, L, D) and not h.requires_grad
    assert torch.equal(o1.hidden_states[-1], o1.last_hidden_state.detach()) and torch.equal(o1.hidden_states[0], x0)


class _Pair(torch.nn.Module):
    """What text_to_patch_attention reads of an AlproBaseModel: the text encoder and the text pass (AlproForSequenceClassification's, whose
    text_encoder is the bare BertModel)."""

    def __init__(self, bert):
        super().__init__()
        self.text_encoder = bert

    def _text_embeds(self, input_ids, attention_mask):
        from alpro_amd.modeling.alpro_models import AlproForSequenceClassification
        return AlproForSequenceClassification._text_embeds(self, input_ids, attention_mask)


@pytest.mark.parametrize("layers", ((-1,), (0, 1)))
def test_text_to_patch_attention_is_the_mean_of_the_full_maps_slice(model, layers):
    from alpro_amd import config as rt
    from alpro_amd.grounding import text_to_patch_attention
    m, ids, mask, emb, att = model
    video = emb[:, LT:].contiguous()
    pair = _Pair(m).eval()
    with rt.use_compute_dtype("fp16"), torch.no_grad():
        got = text_to_patch_attention(pair, ids, mask, video, layers=layers)
        te = m(ids, attention_mask=mask, mode="text").last_hidden_state
        full = m(encoder_embeds=torch.cat([te, video], dim=1), attention_mask=att, mode="fusion", output_attentions=True).attentions
    hg = math.isqrt(LV - 1)
    assert got.shape == (B, LT, hg, hg) and got.dtype == torch.float32
    want = torch.stack([full[i][:, :, :LT, LT + 1:].double().mean(dim=1) for i in layers]).mean(dim=0).view(B, LT, hg, hg)
    # the same fp32 probabilities on both sides (a window is bitwise a slice); only the order of the 12-head and layer sums differs: <= 14 fp32 roundings of values <= 1
    assert float((got.double() - want).abs().max()) <= 14 * 2.0 ** -24
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
        text_to_patch_attention(pair.train(), ids, mask, video)
    pair.eval()
    with pytest.raises(ValueError, match="outside the 2 fusion layers"):
        text_to_patch_attention(pair, ids, mask, video, layers=(2,))
