"""GPU: the models at frame counts that do not divide 32 (temporal attention on attention_temporal_any.hip) against reference-generated
fixtures (tests/golden/make_golden_frames.py): a 12-frame retrieval fine-tune step, pretraining (prompter pass included) at 6 frames and the
visual encoder alone at 48 frames; plus score_all_pairs at 12 frames and QA at 24 frames.  Closed-form weights and inputs as in
tests/golden/parity_cases.py; the tolerances of tests/test_long_text_parity.py and tests/test_model_parity.py for the same quantities."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.test_host_cpu import VENC, make_cfg
from tests.test_long_text_parity import _build, _grad_norm_rel
from tests.test_model_parity import argmax_multinomial, arm_scale, backward, close

pytestmark = pytest.mark.gpu

VIT_ROWS = [0, 1, 100, 196]   # make_golden_frames.VIT_ROWS


def vit_probe(rows):
    """R of the fixed scalar sum(video_embeds * R) (make_golden_frames.vit_probe)."""
    from tests.golden.det_init import unit_uniform
    return torch.from_numpy(unit_uniform("frames/vit_probe", rows * 768).astype(np.float32)).view(1, rows, 768)


EMB_TOL = {"fp32": 1e-3, "bf16": 6e-2, "fp16": 6e-3}   # test_model_parity.test_retrieval_vs_reference's video_embeds tolerances


@pytest.fixture(scope="module")
def retrieval12(bert_cfg):
    m, batch = _build("AlproForVideoTextRetrieval", bert_cfg, 12, 2, 40, "retrieval_frames_T12", False)
    return m, batch, np.load(os.path.join(GOLDEN, "retrieval_T12_B2.npz"))


@pytest.fixture(scope="module")
def pretrain6(bert_cfg):
    m, batch = _build("AlproForPretrain", bert_cfg, 6, 2, 30, "pretrain_release", True)
    return m, batch, np.load(os.path.join(GOLDEN, "pretrain_T6_B2.npz"))


@pytest.fixture(scope="module")
def vit48(bert_cfg):
    m, batch = _build("AlproForVideoTextRetrieval", bert_cfg, 48, 1, 40, "vit_frames_T48", False)
    return m.visual_encoder, batch, np.load(os.path.join(GOLDEN, "vit_T48_B1.npz"))


@pytest.mark.parametrize("mode,tol_logit", [("fp32", 1e-3), ("bf16", 1.6e-2), ("fp16", 2e-3)])
def test_retrieval_T12_vs_reference(retrieval12, monkeypatch, mode, tol_logit):
    """AlproForVideoTextRetrieval at 12 frames: forward, visual embeddings, 1-video x B-captions forward_inference, VTC logits.  fp16 runs
    with the precise [CLS] rows (the default)."""
    from alpro_amd import config as rt
    m, batch, g = retrieval12
    monkeypatch.setattr(torch, "multinomial", argmax_multinomial)
    with rt.use_compute_dtype(mode), torch.no_grad():
        out = m(batch)
        inf = m.forward_inference(dict(visual_inputs=batch["visual_inputs"][:1], text_input_ids=batch["text_input_ids"],
                                       text_input_mask=batch["text_input_mask"]))
        ve, vf = m.encode_video(batch["visual_inputs"])
        _, tf = m.encode_text(batch["text_input_ids"], batch["text_input_mask"])
        sim = vf @ tf.t() / m.temp
    e = {}
    for k in ("itc_loss", "itm_loss", "itm_scores"):
        e[k] = close(out[k], g[k], tol_logit, what=k)
    assert torch.equal(out["itm_labels"].cpu(), torch.from_numpy(g["itm_labels"]).long())
    e["video_embeds"] = close(ve[:, VIT_ROWS], g["video_embeds_rows"], EMB_TOL[mode], what="video_embeds rows (12 frames)")
    close(ve.norm(dim=-1), g["video_embeds_rownorm"], EMB_TOL[mode] * 10, what="video_embeds norms (12 frames)")
    e["inf_itc_scores"] = close(inf["itc_scores"], g["inf_itc_scores"], min(tol_logit, 1e-3) if mode != "bf16" else tol_logit,
                                what="VTC logits (1 video x n captions, 12 frames)")
    e["inf_logits"] = close(inf["logits"], g["inf_logits"], tol_logit, what="inference ITM logits (12 frames)")
    e["sim_v2t"] = close(sim, g["sim_v2t"], min(tol_logit, 1e-3) if mode != "bf16" else tol_logit, what="sim_v2t (12 frames)")
    print("\n[retrieval T=12 %s] max abs errors vs reference:" % mode, {k: "%.2e" % v for k, v in e.items()})


@pytest.mark.parametrize("mode,rtol", [("fp32", 5e-3), ("bf16", 4e-2), ("fp16", 1e-2)])
def test_retrieval_T12_finetune_gradients_vs_reference(retrieval12, monkeypatch, mode, rtol):
    """Retrieval fine-tune step at 12 frames: itm_loss + itc_loss backward through the windowed temporal-attention backward; gradient norms of
    every parameter and full gradients of time_embed and the first and last temporal qkv biases."""
    from alpro_amd import config as rt
    m, batch, g = retrieval12
    for p in m.parameters():
        p.grad = None
    monkeypatch.setattr(torch, "multinomial", argmax_multinomial)
    with rt.use_compute_dtype(mode):
        keep = arm_scale(mode)
        out = m(batch)
        gs = backward(out["itm_loss"] + out["itc_loss"], mode)
        del keep
    tol = {"fp32": 1e-3, "fp16": 2e-3, "bf16": 1.6e-2}[mode]
    for k in ("itc_loss", "itm_loss", "itm_scores"):
        close(out[k], g[k], tol, what=k + " (train graph)")
    names, rel, pd = _grad_norm_rel(m, g, gs)
    print("\n[retrieval T=12 grad parity %s] worst grad-norm rel err %.2e at %s; median %.2e" % (mode, rel.max(), names[int(rel.argmax())], np.median(rel)))
    assert rel.max() < rtol, (names[int(rel.argmax())], float(rel.max()))
    for k in g.files:
        if k.startswith("grad/"):
            r = g[k].astype(np.float64)
            e = np.abs(pd[k[5:]].grad.float().cpu().numpy().astype(np.float64) / gs - r).max()
            scale = max(np.abs(r).max(), 0.5 if k == "grad/temp" else 1e-6)   # temp: its cancelling sum against the non-cancelling scale
            assert e <= rtol * scale + 1e-7, (k, e, np.abs(r).max())


@pytest.mark.parametrize("mode,tol,rtol", [("fp32", 1e-3, 5e-3), ("fp16", 4e-3, 6e-3), ("bf16", 3e-2, 4e-2)])
def test_pretrain_T6_vs_reference(pretrain6, monkeypatch, mode, tol, rtol):
    """AlproForPretrain at the released geometry with 6 frames (the prompter's pseudo labels from a 6-frame pass): losses, ITM scores, MLM
    columns, VTC logits, gradient norms."""
    from alpro_amd import config as rt
    m, batch, g = pretrain6
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
    err = close(vf @ tf.t() / m.temp, g["sim_v2t"], {"fp32": 1e-3, "fp16": 1e-3, "bf16": 1.6e-2}[mode], what="VTC logits (6 frames)")
    close(ve[:, [0, 1, 57, 196]], g["video_embeds_rows"], tol * (1 if mode == "fp32" else 2), what="video_embeds rows (6 frames)")
    close(te[:, [0, 1, 29]], g["text_embeds_rows"], tol * (1 if mode == "fp32" else 2), what="text_embeds rows")
    assert torch.equal(out["itm_labels"].cpu(), torch.from_numpy(g["itm_labels"]).long())
    names, rel, _ = _grad_norm_rel(m, g, gs)
    print("\n[pretrain T=6 %s] VTC logit err %.2e; worst grad-norm rel err %.2e at %s; median %.2e" % (mode, err, rel.max(), names[int(rel.argmax())],
                                                                                                   np.median(rel)))
    assert rel.max() < rtol, (names[int(rel.argmax())], float(rel.max()))


@pytest.mark.parametrize("mode,rtol", [("fp32", 5e-3), ("bf16", 4e-2), ("fp16", 1e-2)])
def test_vit_T48_vs_reference(vit48, mode, rtol):
    """The visual encoder alone at 48 frames (temporal windows of up to 5 tiles): pooled features, rows and row norms of video_embeds, and
    the parameter-gradient norms of sum(video_embeds * R)."""
    from alpro_amd import config as rt
    enc, batch, g = vit48
    for p in enc.parameters():
        p.grad = None
    x = batch["visual_inputs"].transpose(1, 2)
    with rt.use_compute_dtype(mode):
        keep = arm_scale(mode)
        ve = enc.forward_features(x, return_all_tokens=True)
        # 2^-10 (exact): the fixed fp16 test scale 4096 on a sum over 197 x 768 outputs would overflow 16-bit gradients; divided out below
        gs = backward((ve.float() * vit_probe(ve.shape[1]).cuda()).sum() * 2.0 ** -10, mode) * 2.0 ** -10
        del keep
    tol = EMB_TOL[mode]
    e = close(ve[:, 0], g["pooled"], tol, what="pooled features (48 frames)")
    close(ve[:, VIT_ROWS], g["video_embeds_rows"], tol, what="video_embeds rows (48 frames)")
    close(ve.norm(dim=-1), g["video_embeds_rownorm"], tol * 10, what="video_embeds norms (48 frames)")
    pd = dict(enc.named_parameters())
    names = [str(n) for n in g["grad_norm_names"]]
    assert not [n for n in names if pd[n].grad is None]
    got = np.array([float(pd[n].grad.norm()) / gs for n in names])
    rel = np.abs(got - g["grad_norms"]) / np.maximum(g["grad_norms"], 1e-5)
    print("\n[vit T=48 %s] pooled err %.2e; worst grad-norm rel err %.2e at %s; median %.2e" % (mode, e, rel.max(), names[int(rel.argmax())], np.median(rel)))
    assert rel.max() < rtol, (names[int(rel.argmax())], float(rel.max()))
    r = g["grad/model.time_embed"].astype(np.float64)
    d = np.abs(pd["model.time_embed"].grad.float().cpu().numpy().astype(np.float64) / gs - r).max()
    assert d <= rtol * np.abs(r).max(), (d, np.abs(r).max())


def test_score_all_pairs_T12_equals_forward_inference(bert_cfg):
    """retrieval_eval.score_all_pairs (every video / caption encoded once) against forward_inference on the same pairs, at 12 frames."""
    from alpro_amd import config as rt
    from alpro_amd.retrieval_eval import score_all_pairs
    m, batch = _build("AlproForVideoTextRetrieval", bert_cfg, 12, 3, 40, "retrieval_frames_eval", False)
    ids, mask = batch["text_input_ids"], batch["text_input_mask"]
    with rt.use_compute_dtype("fp32"), torch.no_grad():
        score, sim = score_all_pairs(m, batch["visual_inputs"], ids, mask, pair_bsz=4)
        for v in range(3):
            out = m.forward_inference(dict(visual_inputs=batch["visual_inputs"][v:v + 1], text_input_ids=ids, text_input_mask=mask))
            p = torch.softmax(out["logits"].float(), 1)[:, 1]
            assert (score[v] - p).abs().max().item() <= 2e-4
            assert (sim[v] - out["itc_scores"].float().reshape(-1)).abs().max().item() <= 2e-4


def test_qa_T24_fp16_agrees_with_fp32(bert_cfg):
    """AlproForSequenceClassification at 24 frames: encode_clips + answer_logits in fp16 (precise [CLS]) against the exact fp32 mode on the
    same weights and inputs, within the QA logit tolerance of fp16 (tests/test_qa_parity.LOGIT_TOL)."""
    from alpro_amd import config as rt
    from alpro_amd.modeling.alpro_models import AlproForSequenceClassification
    from tests.golden.det_init import det_batch, fill_state_dict_
    from tests.test_qa_parity import LOGIT_TOL, QA_KW
    m = AlproForSequenceClassification(make_cfg(bert_cfg, **QA_KW), dict(VENC, num_frm=24))
    fill_state_dict_(m)
    m.eval().cuda()
    B = 2
    batch = det_batch(B, 24, Lt=40, seed_name="qa_frames_T24", with_mlm=False, with_mpm=False)
    vis, ids, mask = batch["visual_inputs"].cuda(), batch["text_input_ids"].cuda(), batch["text_input_mask"].cuda()
    labels = torch.tensor([3, 1499], dtype=torch.long, device="cuda")
    ti = torch.arange(B, device="cuda")
    res = {}
    for mode in ("fp32", "fp16"):
        with rt.use_compute_dtype(mode), torch.no_grad():
            ve = m.encode_clips(vis)
            te = m.encode_questions(ids, mask)
            logits, loss = m.answer_logits(te, mask, ve, ti, ti, labels)
        assert torch.isfinite(logits).all() and torch.isfinite(loss).all(), mode
        res[mode] = (logits.float().cpu(), loss.float().cpu())
    close(res["fp16"][0], res["fp32"][0].numpy(), LOGIT_TOL["fp16"], what="QA logits (24 frames), fp16 vs fp32")
    close(res["fp16"][1], res["fp32"][1].numpy(), LOGIT_TOL["fp16"], what="QA loss (24 frames), fp16 vs fp32")
