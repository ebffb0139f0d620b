"""GPU: BertModel's output_attentions / output_hidden_states against the REFERENCE's own (tests/golden/bert_attn_B2.npz, written by
tests/golden/make_golden_attn.py from the reference's xbert.BertModel on CPU in fp32): text mode on two 8-token captions, one with two padded
positions, and fusion mode on [text output ; a video [CLS] + 2 x 2 patches], L = 13 -- every attention map, and of every hidden state the rows
{0, last valid text row, first video row}.  Tolerances: the project's 2e-4 (fp32) / 8e-4 (fp16) of max |reference| (tests/test_model_parity.py)."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import BERT_CFG, GOLDEN
from tests.golden import make_golden_attn as ga
from tests.test_host_cpu import make_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bert():
    from alpro_amd.modeling.xbert import BertModel
    m = ga.apply_gain(BertModel(make_cfg(dict(BERT_CFG, **ga.OVERRIDES)), add_pooling_layer=False)).eval().cuda()
    ids, mask, video = ga.case_inputs()
    return m, ids.cuda(), mask.cuda(), video.cuda(), np.load(os.path.join(GOLDEN, ga.FNAME))


def _close(got, ref, tol, what):
    got, ref = got.detach().float().cpu().numpy().astype(np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, lim = float(np.abs(got - ref).max()), tol * float(np.abs(ref).max())
    print("[attn parity] %s: max err %.3e (limit %.3e = %.0e of max |ref| %.3f)" % (what, err, lim, tol, np.abs(ref).max()))
    return err, lim, what


@pytest.mark.parametrize("mode,tol", [("fp32", 2e-4), ("fp16", 8e-4)])
def test_attentions_and_hidden_states_vs_reference(bert, mode, tol):
    from alpro_amd import config as rt
    m, ids, mask, video, g = bert
    with rt.use_compute_dtype(mode), torch.no_grad():
        t = m(ids, attention_mask=mask, return_dict=True, mode="text", output_attentions=True, output_hidden_states=True)
        emb = torch.cat([t.last_hidden_state, video], dim=1)
        att = torch.cat([mask, torch.ones(ga.B, ga.LV, dtype=torch.long, device="cuda")], dim=1)
        f = m(encoder_embeds=emb, attention_mask=att, return_dict=True, mode="fusion", output_attentions=True, output_hidden_states=True)
    res = []
    for name, o, L in (("text", t, ga.LT), ("fusion", f, ga.LT + ga.LV)):
        assert len(o.attentions) == 2 and len(o.hidden_states) == 3
        for i, a in enumerate(o.attentions):
            assert a.shape == (ga.B, 12, L, L) and a.dtype == torch.float32 and not a.requires_grad
            res.append(_close(a, g["%s/attn_%d" % (name, i)], tol, "%s attentions[%d] (%s)" % (name, i, mode)))
            assert float(a[1, :, :, ga.LAST_VALID[1] + 1:ga.LT].max()) == 0.0       # padded keys get exactly nothing (exp(-10000) in fp32)
        for h in o.hidden_states:
            assert h.shape == (ga.B, L, ga.D) and h.dtype == torch.float32 and not h.requires_grad
        res.append(_close(ga.hidden_rows(o.hidden_states, name == "fusion"), g["%s/hidden" % name], tol, "%s hidden_states rows (%s)" % (name, mode)))
        res.append(_close(ga.hidden_rows((o.last_hidden_state,), name == "fusion")[0], g["%s/last_rows" % name], tol, "%s last_hidden_state rows (%s)" % (name, mode)))
        assert torch.equal(o.hidden_states[-1], o.last_hidden_state)
    bad = ["%s: %.3e > %.3e" % (w, e, l) for e, l, w in res if not e <= l]
    assert not bad, bad
