"""GPU: the models with captions long enough to take attention past 256 tokens (attention_long.hip) against reference-generated fixtures
(tests/golden/make_golden_long.py): pretraining at 96-token captions (fusion length 293) and retrieval at 320-token captions (text encoder at
L = 320, fusion at 517).  Closed-form weights and inputs as in tests/golden/parity_cases.py; the tolerances of tests/test_model_parity.py."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.test_host_cpu import VENC, make_cfg
from tests.test_model_parity import argmax_multinomial, arm_scale, backward, close

pytestmark = pytest.mark.gpu


def _build(cls_name, bert_cfg, T, B, Lt, seed, full):
    from alpro_amd.modeling import alpro_models as am
    from tests.golden.det_init import det_batch, fill_state_dict_
    m = getattr(am, cls_name)(make_cfg(bert_cfg), dict(VENC, num_frm=T))
    fill_state_dict_(m)
    m.eval().cuda()
    batch = det_batch(B, T, Lt=Lt, seed_name=seed, with_mlm=full, with_mpm=full)
    return m, {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}


@pytest.fixture(scope="module")
def pretrain96(bert_cfg):
    m, batch = _build("AlproForPretrain", bert_cfg, 4, 2, 96, "pretrain_release", True)
    return m, batch, np.load(os.path.join(GOLDEN, "pretrain_T4_L96_B2.npz"))


@pytest.fixture(scope="module")
def retrieval320(bert_cfg):
    m, batch = _build("AlproForVideoTextRetrieval", bert_cfg, 2, 2, 320, "retrieval_long", False)
    return m, batch, np.load(os.path.join(GOLDEN, "retrieval_T2_B2_L320.npz"))


def _grad_norm_rel(m, g, gs):
    pd = dict(m.named_parameters())
    names = [str(n) for n in g["grad_norm_names"]]
    assert not [n for n in names if pd[n].grad is None]
    got = np.array([float(pd[n].grad.norm()) / gs for n in names])
    ref = g["grad_norms"]
    # temp: one cancelling scalar, measured against the non-cancelling scale; key.bias: identically 0 in exact arithmetic (test_model_parity.py)
    rel = np.abs(got - ref) / np.where(np.array([n == "temp" for n in names]), np.maximum(ref, 0.5), np.maximum(ref, 1e-5))
    zero_grad = np.array([n.endswith("attention.self.key.bias") for n in names])
    assert got[zero_grad].max() < 1e-3
    rel[zero_grad] = 0.0
    return names, rel, pd


@pytest.mark.parametrize("mode,tol,rtol", [("fp32", 1e-3, 5e-3), ("fp16", 4e-3, 6e-3), ("bf16", 3e-2, 4e-2)])
def test_pretrain_L96_vs_reference(pretrain96, monkeypatch, mode, tol, rtol):
    """AlproForPretrain, 4 frames x 96 tokens (fusion L = 293): losses, ITM scores, MLM columns, VTC logits, gradient norms."""
    from alpro_amd import config as rt
    m, batch, g = pretrain96
    for p in m.parameters():
        p.grad = None
    monkeypatch.setattr(torch, "multinomial", argmax_multinomial)
    with rt.use_compute_dtype(mode):
        with torch.no_grad():
            ve = m._forward_visual_embeds(batch["visual_inputs"])
            te, tf = m._forward_text_feats(batch)
            vf = m._video_feat(ve)
        keep = arm_scale(mode)
        out = m(batch)
        gs = backward(out["mlm_loss"] + out["itm_loss"] + out["itc_loss"] + out["mpm_loss"], mode)
        del keep
    for k in ("itc_loss", "itm_loss", "mlm_loss", "mpm_loss", "itm_scores", "mpm_logits"):
        close(out[k], g[k], tol, what=k)
    close(out["mlm_scores"][:, :, ::61], g["mlm_scores_cols"], tol, what="mlm_scores")
    err = close(vf @ tf.t() / m.temp, g["sim_v2t"], {"fp32": 1e-3, "fp16": 1e-3, "bf16": 1.6e-2}[mode], what="VTC logits (Lt = 96)")
    close(te[:, [0, 1, 29]], g["text_embeds_rows"], tol * (1 if mode == "fp32" else 2), what="text_embeds rows")
    assert torch.equal(out["itm_labels"].cpu(), torch.from_numpy(g["itm_labels"]).long())
    names, rel, _ = _grad_norm_rel(m, g, gs)
    print("\n[long pretrain %s] VTC logit err %.2e; worst grad-norm rel err %.2e at %s; median %.2e" % (mode, err, rel.max(), names[int(rel.argmax())],
                                                                                                    np.median(rel)))
    assert rel.max() < rtol, (names[int(rel.argmax())], float(rel.max()))


@pytest.mark.parametrize("mode,tol_logit", [("fp32", 1e-3), ("bf16", 1.6e-2), ("fp16", 2e-3)])
def test_retrieval_L320_vs_reference(retrieval320, monkeypatch, mode, tol_logit):
    """AlproForVideoTextRetrieval, 320-token captions (text L = 320, fusion L = 517): forward, 1-video x B-captions forward_inference, VTC
    logits.  fp16 runs with the precise [CLS] rows (the default), i.e. through the long kernel's CLS query."""
    from alpro_amd import config as rt
    m, batch, g = retrieval320
    monkeypatch.setattr(torch, "multinomial", argmax_multinomial)
    with rt.use_compute_dtype(mode), torch.no_grad():
        out = m(batch)
        inf = m.forward_inference(dict(visual_inputs=batch["visual_inputs"][:1], text_input_ids=batch["text_input_ids"],
                                       text_input_mask=batch["text_input_mask"]))
        _, vf = m.encode_video(batch["visual_inputs"])
        _, tf = m.encode_text(batch["text_input_ids"], batch["text_input_mask"])
        sim = vf @ tf.t() / m.temp
    e = {}
    for k in ("itc_loss", "itm_loss", "itm_scores"):
        e[k] = close(out[k], g[k], tol_logit, what=k)
    e["inf_itc_scores"] = close(inf["itc_scores"], g["inf_itc_scores"], min(tol_logit, 1e-3) if mode != "bf16" else tol_logit,
                                what="VTC logits (1 video x n captions, Lt = 320)")
    e["inf_logits"] = close(inf["logits"], g["inf_logits"], tol_logit, what="inference ITM logits")
    e["sim_v2t"] = close(sim, g["sim_v2t"], min(tol_logit, 1e-3) if mode != "bf16" else tol_logit, what="sim_v2t")
    assert torch.equal(out["itm_labels"].cpu(), torch.from_numpy(g["itm_labels"]).long())
    print("\n[long retrieval %s] max abs errors vs reference:" % mode, {k: "%.2e" % v for k, v in e.items()})
    if mode == "fp16":
        print("[long retrieval fp16 + precise CLS] VTC logit error %.2e (north star 1e-3)" % max(e["inf_itc_scores"], e["sim_v2t"]))


@pytest.mark.parametrize("mode,rtol", [("fp32", 5e-3), ("bf16", 4e-2), ("fp16", 1e-2)])
def test_retrieval_L320_finetune_gradients_vs_reference(retrieval320, monkeypatch, mode, rtol):
    """Retrieval finetune step at 320-token captions: loss = itm_loss + itc_loss backward through the long attention backward."""
    from alpro_amd import config as rt
    m, batch, g = retrieval320
    for p in m.parameters():
        p.grad = None
    monkeypatch.setattr(torch, "multinomial", argmax_multinomial)
    with rt.use_compute_dtype(mode):
        out = m(batch)
        gs = backward(out["itm_loss"] + out["itc_loss"], mode)
    tol = {"fp32": 1e-3, "fp16": 2e-3, "bf16": 1.6e-2}[mode]
    for k in ("itc_loss", "itm_loss", "itm_scores"):
        close(out[k], g[k], tol, what=k + " (train graph)")
    names, rel, pd = _grad_norm_rel(m, g, gs)
    print("\n[long retrieval grad parity %s] worst grad-norm rel err %.2e at %s; median %.2e" % (mode, rel.max(), names[int(rel.argmax())], np.median(rel)))
    assert rel.max() < rtol, (names[int(rel.argmax())], float(rel.max()))
    for k in g.files:
        if k.startswith("grad/"):
            r = g[k].astype(np.float64)
            e = np.abs(pd[k[5:]].grad.float().cpu().numpy().astype(np.float64) / gs - r).max()
            if k.endswith("attention.self.key.bias"):   # 0 in exact arithmetic: an absolute bound, as for its norm above
                assert e < 1e-3, (k, e)
                continue
            # temp: its cancelling sum is measured against the non-cancelling scale, as for its norm above
            scale = max(np.abs(r).max(), 0.5 if k == "grad/temp" else 1e-6)
            assert e <= rtol * scale + 1e-7, (k, e, np.abs(r).max())


def test_score_all_pairs_L96_equals_forward_inference(bert_cfg):
    """retrieval_eval.score_all_pairs (every video / caption encoded once, flat fusion mini-batches at L = 96 + 197) against forward_inference
    on the same (video, caption) pairs."""
    from alpro_amd import config as rt
    from alpro_amd.retrieval_eval import score_all_pairs
    m, batch = _build("AlproForVideoTextRetrieval", bert_cfg, 2, 3, 96, "retrieval_long_eval", False)
    ids, mask = batch["text_input_ids"], batch["text_input_mask"]
    with rt.use_compute_dtype("fp32"), torch.no_grad():
        score, sim = score_all_pairs(m, batch["visual_inputs"], ids, mask, pair_bsz=4)
        for v in range(3):
            out = m.forward_inference(dict(visual_inputs=batch["visual_inputs"][v:v + 1], text_input_ids=ids, text_input_mask=mask))
            p = torch.softmax(out["logits"].float(), 1)[:, 1]
            assert (score[v] - p).abs().max().item() <= 2e-4
            assert (sim[v] - out["itc_scores"].float().reshape(-1)).abs().max().item() <= 2e-4
