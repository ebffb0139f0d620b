"""GPU: the Grad-CAM path against the REFERENCE's own autograd (tests/golden/bert_gradcam_B2.npz, written by tests/golden/make_golden_gradcam.py
from the reference's xbert.BertModel on CPU in fp32 with .retain_grad() on both fusion `attentions`): the case of
tests/test_attn_outputs_parity.py -- two 8-token captions, one with two padded positions, fused with a video [CLS] + 2 x 2 patches, L = 13 --
a closed-form 768 -> 2 head on the fusion [CLS] row, score = logits[:, 1].sum().  Compared: G = d(score) / d(attention_probs) and
CAM = P * relu(G) of both fusion layers, the logits, d(score) / d(video tokens), and grounding.text_to_patch_gradcam (8 tokens x 2 x 2 patches).
Limits, of max |reference|: 2e-4 (fp32, the exact mode) and 1e-2 (fp16 gradients, tests/test_model_parity.py)."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import BERT_CFG, GOLDEN
from tests.golden import make_golden_attn as ga
from tests.golden import make_golden_gradcam as gg
from tests.test_gradcam_gpu import SCALE, TOL, PairITM, scaled_backward
from tests.test_host_cpu import make_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    from alpro_amd.modeling.xbert import BertModel
    m = ga.apply_gain(BertModel(make_cfg(dict(BERT_CFG, **ga.OVERRIDES)), add_pooling_layer=False)).eval().cuda()
    ids, mask, video = ga.case_inputs()
    return PairITM(m, gg.head().cuda()).eval(), ids.cuda(), mask.cuda(), video.cuda(), np.load(os.path.join(GOLDEN, gg.FNAME))


def _close(got, ref, tol, what):
    got, ref = got.detach().float().cpu().numpy().astype(np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, lim = float(np.abs(got - ref).max()), tol * float(np.abs(ref).max())
    print("[gradcam parity] %s: max err %.3e = %.3e of max |ref| %.3e (limit %.0e)" % (what, err, err / np.abs(ref).max(), np.abs(ref).max(), tol))
    return err, lim, what


@pytest.mark.parametrize("mode", ("fp32", "fp16"))
def test_gradients_cams_and_the_helper_vs_reference(case, mode):
    from alpro_amd import config as rt
    from alpro_amd.grounding import text_to_patch_gradcam
    from alpro_amd.modeling.alpro_models import _linear32
    from alpro_amd.modeling.xbert import AttnGradients
    pair, ids, mask, video, g = case
    m, tol = pair.text_encoder, TOL[mode]
    col = AttnGradients(want=("grad", "cam"), grad_scale=SCALE[mode])
    with rt.use_compute_dtype(mode):
        with torch.no_grad():
            te = pair._text_embeds(ids, mask)
        v = video.clone().requires_grad_(True)
        att = torch.cat([mask, torch.ones(ga.B, ga.LV, dtype=torch.long, device="cuda")], dim=1)
        o = m(encoder_embeds=torch.cat([te, v], dim=1), attention_mask=att, return_dict=True, mode="fusion", attn_grads=col)
        logits = _linear32(o.last_hidden_state[:, 0, :], pair.itm_head)
        s = scaled_backward(logits[:, 1].sum(), mode)
        helper = text_to_patch_gradcam(pair, ids, mask, video, layers=(0, 1))
    for p in pair.parameters():
        p.grad = None
    res = [_close(logits, g["logits"], {"fp32": 2e-4, "fp16": 8e-4}[mode], "logits (%s)" % mode),
           _close(v.grad[:, list(gg.VIDEO_ROWS)] / s, g["d_video"], tol, "d score / d video tokens (%s)" % mode)]
    cams = []
    for i in range(2):
        ref_g, ref_p = g["fusion/grad_%d" % i], g["fusion/attn_%d" % i]
        cams.append(ref_p.astype(np.float64) * np.maximum(ref_g.astype(np.float64), 0.0))
        assert col.grads[i].shape == (ga.B, 12, ga.LT + ga.LV, ga.LT + ga.LV)
        res.append(_close(col.grads[i], ref_g, tol, "fusion G[%d] (%s)" % (i, mode)))
        res.append(_close(col.cams[i], cams[i], tol, "fusion CAM[%d] (%s)" % (i, mode)))
    want = np.mean([c[:, :, :ga.LT, ga.LT + 1:].mean(axis=1) for c in cams], axis=0).reshape(ga.B, ga.LT, 2, 2)
    assert helper.shape == (ga.B, ga.LT, 2, 2) and float(helper.max()) > 0
    res.append(_close(helper, want, tol, "text_to_patch_gradcam layers (0, 1) (%s)" % mode))
    bad = ["%s: %.3e > %.3e" % (w, e, l) for e, l, w in res if not e <= l]
    assert not bad, bad
