"""Golden vectors for the Grad-CAM path (BertModel.forward attn_grads, grounding.text_to_patch_gradcam), from the REFERENCE itself (CPU, fp32,
eval, torch autograd).

    python -m tests.golden.make_golden_gradcam          # writes tests/golden/bert_gradcam_B2.npz

The case of make_golden_attn.py (its inputs, its weights, its QK_GAIN): the reference's xbert.BertModel runs the text pass without grad and the
fusion pass over [text output ; 5 video tokens] WITH grad, the video tokens being the leaf.  A closed-form 768 -> 2 head (det_init, weight times
HEAD_GAIN) stands for itm_head; score = logits[:, 1].sum(); both fusion `attentions` carry .retain_grad(), so after score.backward() their
.grad is d(score) / d(attention_probs) -- what the reference's own save_attn_gradients hook receives (xbert.py:325-327).  Stored:
  fusion/grad_<i>, fusion/attn_<i> (2, 12, 13, 13), logits (2, 2), d_video (2, 3, 768): d(score) / d(video tokens), rows {0, 1, 4}.
head() and the row choice need no reference: tests/test_gradcam_parity.py builds the same case from them.  The reference is needed only by
main(); it never runs on the GPU box.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.det_init import det_param  # noqa: E402
from tests.golden.make_golden_attn import B, D, LT, LV, OVERRIDES, apply_gain, case_inputs  # noqa: E402

FNAME = "bert_gradcam_B2.npz"
HEAD_GAIN = 1.0          # raised if a map fails a floor below (see main)
VIDEO_ROWS = (0, 1, 4)   # the video [CLS], the first and the last patch token


def head():
    """The stand-in for itm_head: nn.Linear(768, 2) with closed-form values."""
    lin = torch.nn.Linear(D, 2)
    with torch.no_grad():
        lin.weight.copy_(det_param("gradcam_golden/itm_head.weight", (2, D)) * HEAD_GAIN)
        lin.bias.copy_(det_param("gradcam_golden/itm_head.bias", (2,)))
    return lin


def main():
    from tests.golden import ref_harness as rh
    _, xbert = rh.import_reference()
    cfg, _ = rh.make_configs(**OVERRIDES)
    m = apply_gain(xbert.BertModel(cfg, add_pooling_layer=False)).eval()
    lin = head()
    ids, mask, video = case_inputs()
    with torch.no_grad():
        t = m(ids, attention_mask=mask, return_dict=True, mode="text")
    video = video.clone().requires_grad_(True)
    emb = torch.cat([t.last_hidden_state, video], dim=1)
    att = torch.cat([mask, torch.ones(B, LV, dtype=torch.long)], dim=1)
    f = m(encoder_embeds=emb, attention_mask=att, return_dict=True, mode="fusion", output_attentions=True)
    assert len(f.attentions) == 2
    for a in f.attentions:
        a.retain_grad()
    logits = lin(f.last_hidden_state[:, 0])
    logits[:, 1].sum().backward()
    g = {"logits": logits.detach().numpy().astype(np.float32), "d_video": video.grad[:, list(VIDEO_ROWS)].numpy().astype(np.float32)}
    for i, a in enumerate(f.attentions):
        assert a.shape == (B, 12, LT + LV, LT + LV) and a.grad is not None
        g["fusion/attn_%d" % i] = a.detach().numpy().astype(np.float32)
        g["fusion/grad_%d" % i] = a.grad.numpy().astype(np.float32)
        # the floors that keep the ReLU from emptying a map: some gradient at all, and at least a quarter of the entries positive.  The score
        # reads the fusion [CLS] row only, so in the LAST layer every query row but row 0 has a gradient of exactly zero (12 of 13 rows, on the
        # reference: measured 0.035 of all entries positive = 0.455 of row 0, whatever the head's gain); the quarter is therefore asked of the
        # query rows the score reaches (those with a non-zero entry) -- all 13 in the first layer, where it is the floor on the whole map.
        gr = g["fusion/grad_%d" % i]
        reached = np.abs(gr).max(axis=(0, 1, 3)) > 0
        pos_all, pos = float((gr > 0).mean()), float((gr[:, :, reached] > 0).mean())
        print("fusion/grad_%d: max |G| %.3e, query rows reached %d of %d, share of positive entries %.3f of the map, %.3f of the reached rows"
              % (i, np.abs(gr).max(), int(reached.sum()), reached.size, pos_all, pos))
        assert np.abs(gr).max() > 0, "fusion/grad_%d is identically zero" % i
        assert reached.all() if i == 0 else reached[0], "fusion/grad_%d: the score does not reach the rows it must" % i
        assert pos >= 0.25, "fewer than a quarter of fusion/grad_%d is positive on the rows the score reaches: raise HEAD_GAIN" % i
    p = os.path.join(HERE, FNAME)
    np.savez_compressed(p, **g)
    print(FNAME, os.path.getsize(p), {k: v.shape for k, v in g.items()})


if __name__ == "__main__":
    main()
