"""Golden vectors for video question answering, from the REFERENCE itself (CPU, fp32, eval).

    python -m tests.golden.make_golden_qa          # writes tests/golden/qa_T16_B2.npz, qa_clips_T2_B3_C3.npz

  * qa_T16_B2.npz          AlproForSequenceClassification at the msrvtt_qa geometry (16 frames, 40-token questions with padded tails,
                           num_labels 1500, classifier "mlp", cls_hidden_scale 2; set on the BertConfig as run_video_qa.py:162-167 does):
                           logits and loss of forward(batch), logits of forward with labels=None, gradient norms of every trained tensor
                           and a few full gradients (both classifier biases, a column slice of the answer layer, fusion and visual biases).
                           Labels include 1499, the last answer column.
  * qa_clips_T2_B3_C3.npz  3 questions x 3 clips x 2 frames: the per-clip logits of the reference model run once per clip, as
                           run_video_qa.py:249-258 does, the pooled logits and answers for mean / max / lse and the clip-averaged loss.
                           The pooling is written here in plain torch.
Weights and inputs come from det_init.py closed forms, as in make_golden.py.  Needs the reference; never runs on the GPU box.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import make_golden as mg  # noqa: E402
from tests.golden import ref_harness as rh  # noqa: E402
from tests.golden.det_init import det_batch, fill_state_dict_  # noqa: E402

NUM_LABELS = 1500
QA_LABELS_T16 = [1499, 37]
QA_LABELS_CLIPS = [1499, 0, 702]
QA_GRAD_FULL = ["classifier.0.bias", "classifier.2.bias",
                "text_encoder.encoder.layer.11.output.dense.bias",
                "text_encoder.encoder.layer.8.attention.self.value.bias",
                "text_encoder.encoder.layer.6.attention.output.LayerNorm.bias",
                "visual_encoder.model.blocks.11.mlp.fc2.bias",
                "visual_encoder.model.norm.bias"]
QA_W2_COLS = 16   # classifier.2.weight[:, :QA_W2_COLS]: every answer row, the first hidden columns


def qa_config(T):
    """run_video_qa.py:157-177 for config_release/msrvtt_qa.json: the downstream attributes on the BertConfig, num_frm on the ViT config."""
    cfg, venc = rh.make_configs(num_frm=T)
    for k, v in dict(num_labels=NUM_LABELS, classifier="mlp", cls_hidden_scale=2, loss_type="ce").items():
        setattr(cfg, k, v)
    return cfg, venc


def qa_batch(B, T, seed_name, labels):
    batch = det_batch(B, T, Lt=40, seed_name=seed_name, with_mlm=False, with_mpm=False)
    batch["labels"] = torch.tensor(labels, dtype=torch.long)
    return batch


def case_qa(am, fname, T=16, B=2):
    cfg, venc = qa_config(T)
    m = am.AlproForSequenceClassification(cfg, venc)
    fill_state_dict_(m)
    m.eval()
    batch = qa_batch(B, T, "qa_T16", QA_LABELS_T16)
    out = m(batch)
    g = {"logits": mg.npf(out["logits"]), "loss": mg.npf(out["loss"]), "labels": batch["labels"].numpy()}
    with torch.no_grad():
        nolab = m(dict(batch, labels=None))
    assert nolab["loss"] == 0
    g["logits_nolabels"] = mg.npf(nolab["logits"])
    out["loss"].backward()
    names, norms = [], []
    for n_, p_ in m.named_parameters():
        if p_.grad is not None:
            names.append(n_)
            norms.append(float(p_.grad.norm()))
    g["grad_norm_names"] = np.array(names)
    g["grad_norms"] = np.array(norms, dtype=np.float64)
    pd = dict(m.named_parameters())
    for n_ in QA_GRAD_FULL:
        assert pd[n_].grad is not None, n_
        g["grad/" + n_] = mg.npf(pd[n_].grad)
    g["grad_cols/classifier.2.weight"] = mg.npf(pd["classifier.2.weight"].grad[:, :QA_W2_COLS])
    np.savez_compressed(os.path.join(HERE, fname), **g)


def case_qa_clips(am, fname, T=2, B=3, C=3):
    cfg, venc = qa_config(T)
    m = am.AlproForSequenceClassification(cfg, venc)
    fill_state_dict_(m)
    m.eval()
    batch = qa_batch(B, T * C, "qa_clips", QA_LABELS_CLIPS)
    vis = batch["visual_inputs"].view((B, C, T) + tuple(batch["visual_inputs"].shape[2:]))
    logits, losses = [], []
    with torch.no_grad():
        for c in range(C):   # the whole model once per clip, as the driver does
            out = m(dict(batch, visual_inputs=vis[:, c]))
            logits.append(out["logits"])
            losses.append(float(out["loss"]))
    stacked = torch.stack(logits)                                  # (C, B, A)
    g = {"clip_logits": mg.npf(stacked), "labels": batch["labels"].numpy(), "loss": np.float64(sum(losses) / C)}
    pooled = {"mean": stacked.mean(0), "max": stacked.amax(0), "lse": torch.logsumexp(stacked, dim=0)}
    for k, v in pooled.items():
        g["pooled/" + k] = mg.npf(v)
        g["pred/" + k] = v.argmax(-1).numpy()
    np.savez_compressed(os.path.join(HERE, fname), **g)


def main():
    am, _ = rh.import_reference()
    torch.set_num_threads(8)
    only = set(sys.argv[1:])
    if not only or "qa" in only:
        case_qa(am, "qa_T16_B2.npz")
    if not only or "clips" in only:
        case_qa_clips(am, "qa_clips_T2_B3_C3.npz")
    for f in ("qa_T16_B2.npz", "qa_clips_T2_B3_C3.npz"):
        p = os.path.join(HERE, f)
        if os.path.exists(p):
            print(f, os.path.getsize(p))


if __name__ == "__main__":
    main()
