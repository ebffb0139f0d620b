"""GPU: video question answering (AlproForSequenceClassification, alpro_amd/qa_eval.py) against the REFERENCE's fixtures
(tests/golden/make_golden_qa.py): forward and gradients at the msrvtt_qa geometry in every operand dtype, and multi-clip evaluation with
mean / max / lse pooling; plus the model's own invariants (tail rows on / off, forward_inference, pooled evaluation vs a per-clip loop)."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.test_host_cpu import VENC, make_cfg
from tests.test_model_parity import backward, close, fresh_grads, to_dev

pytestmark = pytest.mark.gpu

LOGIT_TOL = {"fp32": 1e-3, "fp16": 2e-3, "bf16": 1.6e-2}      # test_retrieval_finetune_gradients_vs_reference's logit tolerances
GRAD_RTOL = {"fp32": 5e-3, "fp16": 1e-2, "bf16": 4e-2}        # ... and its gradient rtol
QA_KW = dict(num_labels=1500, classifier="mlp", cls_hidden_scale=2, loss_type="ce")   # run_video_qa.py:162-167 (msrvtt_qa.json)


def _qa_model(bert_cfg, T):
    from alpro_amd.modeling.alpro_models import AlproForSequenceClassification
    from tests.golden.det_init import fill_state_dict_
    m = AlproForSequenceClassification(make_cfg(bert_cfg, **QA_KW), dict(VENC, num_frm=T))
    fill_state_dict_(m)
    return m.eval().cuda()


def _qa_batch(B, T, seed_name, labels):
    from tests.golden.det_init import det_batch
    batch = det_batch(B, T, Lt=40, seed_name=seed_name, with_mlm=False, with_mpm=False)
    batch["labels"] = torch.as_tensor(np.asarray(labels), dtype=torch.long)
    return to_dev(batch)


@pytest.fixture(scope="module")
def qa16(bert_cfg):
    g = np.load(os.path.join(GOLDEN, "qa_T16_B2.npz"))
    return _qa_model(bert_cfg, 16), _qa_batch(2, 16, "qa_T16", g["labels"]), g


@pytest.fixture(scope="module")
def qa_clips(bert_cfg):
    g = np.load(os.path.join(GOLDEN, "qa_clips_T2_B3_C3.npz"))
    batch = _qa_batch(3, 6, "qa_clips", g["labels"])
    batch["question_ids"] = ["q0", "q1", "q2"]
    return _qa_model(bert_cfg, 2), batch, g


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_qa_forward_vs_reference(qa16, mode):
    from alpro_amd import config as rt
    m, batch, g = qa16
    tol = LOGIT_TOL[mode]
    with rt.use_compute_dtype(mode), torch.no_grad():
        out = m(batch)
        nolab = m(dict(batch, labels=None))
    close(out["logits"], g["logits"], tol, what="QA logits (16 frames, 1500 answers)")
    close(out["loss"], g["loss"], tol, what="QA loss")
    close(nolab["logits"], g["logits_nolabels"], tol, what="QA logits, labels=None")
    assert nolab["loss"] == 0


def _spy_relu_gates(monkeypatch):
    """-> a list that receives [H > 0] of the answer MLP's hidden layer (the ReLU launch's output) at every forward from now on."""
    from alpro_amd import hip
    seen, orig = [], hip.gemm_rows

    def spy(*a, **k):
        out = orig(*a, **k)
        if k.get("act") == hip.ACT_RELU:
            seen.append(out > 0)
        return out
    monkeypatch.setattr(hip, "gemm_rows", spy)
    return seen


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_qa_gradients_vs_reference(qa16, mode, monkeypatch):
    """loss.backward() through the answer MLP (ReLU-mask row kernel), the fusion tail on the [CLS] rows, the fusion gather and both encoders:
    gradient norms of every trained tensor and a few full gradients vs the reference, as the retrieval finetune test checks them."""
    from alpro_amd import config as rt
    m, batch, g = qa16
    gates = _spy_relu_gates(monkeypatch)
    with rt.use_compute_dtype("fp32"), torch.no_grad():
        m(batch)
    fresh_grads(m)
    with rt.use_compute_dtype(mode):
        out = m(batch)
        gs = backward(out["loss"], mode)
    # hidden units whose ReLU gate in this backward's forward differs from the exact mode's in some row: their classifier.0.bias entry is a
    # different function of the inputs (the 16-bit [CLS] row moved a pre-activation across 0), so that entry is not compared -- they are few
    flipped = (gates[1] != gates[0]).any(0).cpu().numpy()
    assert len(gates) == 2 and flipped.mean() < 0.02, flipped.sum()
    rtol = GRAD_RTOL[mode]
    close(out["logits"], g["logits"], LOGIT_TOL[mode], what="QA logits (train graph)")
    pd = dict(m.named_parameters())
    if gs != 1.0:
        for p_ in pd.values():
            if p_.grad is not None:
                p_.grad.div_(gs)
    names = [str(n) for n in g["grad_norm_names"]]
    missing = [n for n in names if pd[n].grad is None]
    assert not missing, "no gradient for %s" % missing[:5]
    extra = [n for n, p in pd.items() if p.grad is not None and n not in names]
    assert not extra, "unexpected gradients %s" % extra[:5]
    got = np.array([float(pd[n].grad.norm()) for n in names])
    ref = g["grad_norms"]
    # The fusion layers' query / key gradients pass through the softmax Jacobian, whose rows sum to zero over the keys: with the closed-form
    # weights they are ~20x smaller than the same layer's value gradients (layer 10: key.weight 0.12 against value.weight 2.5), and bf16
    # noise of the value-gradient size lands on them -- 5e-2 of their own norm in layer 10, the same with the tail rows on or off.  Like `temp`
    # in the retrieval test, their error is measured against the non-cancelling scale, the value counterpart's norm.
    scale = {n: r for n, r in zip(names, ref)}
    qk = (".attention.self.query.", ".attention.self.key.")
    floor = np.array([scale.get(n.replace("query", "value").replace("key", "value"), 1e-5) if any(t in n for t in qk) else 1e-5 for n in names])
    rel = np.abs(got - ref) / np.maximum(ref, floor)
    zero_grad = np.array([n.endswith("attention.self.key.bias") for n in names])   # exactly 0 in exact arithmetic (softmax shift invariance)
    assert got[zero_grad].max() < 1e-3
    rel[zero_grad] = 0.0
    worst = int(rel.argmax())
    print("\n[qa grad parity %s] worst grad-norm rel err %.2e at %s; median %.2e" % (mode, rel.max(), names[worst], np.median(rel)))
    assert rel.max() < rtol, (names[worst], got[worst], ref[worst])
    full = {k[5:]: g[k] for k in g.files if k.startswith("grad/")}
    full["classifier.2.weight"] = g["grad_cols/classifier.2.weight"]
    for n, r in full.items():
        if flipped.any() and not n.startswith("classifier."):
            # below the answer MLP every entry of the gradient mixes the flipped units' full-size terms (dX = dH W1): only the norms above
            # compare there; classifier.2 sits before the gate in the backward, classifier.0.bias is compared on the units that did not flip
            print("[qa grad parity %s] %d of %d ReLU units flipped: %s compared by norm only" % (mode, flipped.sum(), flipped.size, n))
            continue
        r = r.astype(np.float64)
        gt = pd[n].grad.float()
        if n == "classifier.2.weight":
            gt = gt[:, :r.shape[1]]
        if n == "classifier.0.bias":
            gt, r = gt[~torch.from_numpy(flipped).to(gt.device)], r[~flipped]
        e = np.abs(gt.cpu().numpy().astype(np.float64) - r).max()
        assert e <= rtol * max(np.abs(r).max(), 1e-6) + 1e-7, (n, e, np.abs(r).max())
    fresh_grads(m)


@pytest.mark.parametrize("agg", ["mean", "max", "lse"])
@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_inference_qa_vs_reference_clips(qa_clips, mode, agg):
    """3 questions x 3 clips x 2 frames: answers and clip-averaged loss of the pooled evaluation vs the reference model run once per clip."""
    from alpro_amd import config as rt
    from alpro_amd.qa_eval import inference_qa
    m, batch, g = qa_clips
    tol = LOGIT_TOL[mode]
    with rt.use_compute_dtype(mode):
        records, loss = inference_qa(m, [batch], num_clips=3, num_frm=2, score_agg_func=agg)
    assert [r["question_id"] for r in records] == batch["question_ids"]
    pred = np.array([r["answer"] for r in records])
    ref_pred, pooled = g["pred/" + agg], g["pooled/" + agg].astype(np.float64)
    if mode == "fp32":
        assert np.array_equal(pred, ref_pred), (pred, ref_pred)
    else:
        top2 = np.sort(pooled, axis=-1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > 2 * tol
        assert np.array_equal(pred[clear], ref_pred[clear]), (pred, ref_pred, clear)
    assert abs(loss - float(g["loss"])) <= tol, (loss, float(g["loss"]))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_per_clip_logits_vs_reference(qa_clips, mode):
    from alpro_amd import config as rt
    m, batch, g = qa_clips
    vis = batch["visual_inputs"].view((3, 3, 2) + tuple(batch["visual_inputs"].shape[2:]))
    with rt.use_compute_dtype(mode), torch.no_grad():
        for c in range(3):
            out = m(dict(batch, visual_inputs=vis[:, c]))
            close(out["logits"], g["clip_logits"][c], LOGIT_TOL[mode], what="clip %d logits" % c)


@pytest.mark.parametrize("mode,tol", [("fp32", 1e-5), ("bf16", 1e-2)])
def test_fusion_tail_rows_on_and_off_agree(qa16, mode, tol):
    from alpro_amd import config as rt
    m, batch, _ = qa16
    with rt.use_compute_dtype(mode), torch.no_grad():
        assert m.fusion_tail_rows
        on = m(batch)
        m.fusion_tail_rows = False
        try:
            off = m(batch)
        finally:
            m.fusion_tail_rows = True
    close(on["logits"], off["logits"].cpu().numpy(), tol, what="logits, tail rows on vs off")
    close(on["loss"], off["loss"].cpu().numpy(), tol, what="loss, tail rows on vs off")


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_forward_inference_equals_forward_logits(qa16, mode):
    from alpro_amd import config as rt
    m, batch, _ = qa16
    with rt.use_compute_dtype(mode), torch.no_grad():
        a = m(batch)["logits"]
        b = m.forward_inference(batch)
    assert torch.equal(a, b)


@pytest.mark.parametrize("agg", ["mean", "max", "lse"])
def test_inference_qa_equals_a_per_clip_loop(qa_clips, agg):
    """The pooled evaluation against the driver's loop (run_video_qa.py:249-276): model(batch) once per clip, torch pooling, argmax."""
    from alpro_amd import config as rt
    from alpro_amd.qa_eval import inference_qa
    m, batch, _ = qa_clips
    C, T = 3, 2
    with rt.use_compute_dtype("fp32"):
        records, loss = inference_qa(m, [batch], num_clips=C, num_frm=T, score_agg_func=agg, clip_chunk=4)
    vis = batch["visual_inputs"].view((3, C, T) + tuple(batch["visual_inputs"].shape[2:]))
    logits, losses = [], []
    with torch.no_grad(), rt.use_compute_dtype("fp32"):
        for c in range(C):
            out = m(dict(batch, visual_inputs=vis[:, c]))
            logits.append(out["logits"].double().cpu())
            losses.append(float(out["loss"]))
    s = torch.stack(logits)
    pooled = {"mean": s.mean(0), "max": s.amax(0), "lse": torch.logsumexp(s, 0)}[agg]
    assert [r["answer"] for r in records] == pooled.argmax(-1).tolist()
    assert abs(loss - sum(losses) / C) <= 1e-4   # fp32 (the 9-pair and 3-pair fusion batches may tile differently; bf16 differs by ~4e-4)


def test_answer_head_beyond_one_row_chunk(qa_clips):
    """More than 512 (question, clip) rows: the head runs the row kernel in chunks; every row equals the same row computed alone."""
    from alpro_amd.modeling.alpro_models import _QAHead
    m, _, _ = qa_clips
    g = torch.Generator().manual_seed(5)
    x = torch.randn(700, 768, generator=g).cuda()
    labels = torch.randint(0, 1500, (700,), generator=g).cuda()
    c0, c2 = m.classifier[0], m.classifier[2]
    with torch.no_grad():
        logits, loss_rows = _QAHead.apply(x, c0.weight, c0.bias, c2.weight, c2.bias, labels)
        ref = torch.relu(x.double() @ c0.weight.double().t() + c0.bias.double()) @ c2.weight.double().t() + c2.bias.double()
        ref_loss = torch.nn.functional.cross_entropy(ref, labels, reduction="none")
    assert (logits.double() - ref).abs().max().item() < 1e-4
    assert (loss_rows.double() - ref_loss).abs().max().item() < 1e-4
