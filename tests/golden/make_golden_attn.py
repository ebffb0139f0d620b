"""Golden vectors for BertModel's output_attentions / output_hidden_states, from the REFERENCE itself (CPU, fp32, eval).

    python -m tests.golden.make_golden_attn          # writes tests/golden/bert_attn_B2.npz

The reference's xbert.BertModel (4 layers, fusion_layer 2, vocabulary cut to 2048 rows, everything else config_release/base_model.json) with the
closed-form weights of det_init.py, run twice with output_attentions=True, output_hidden_states=True:
  * mode 'text' on two 8-token captions, the second with two padded positions -> text/attn_<i> (2, 12, 8, 8), text/hidden (3, 2, 2, 768): of
    every hidden state the rows {0, last valid text row};
  * mode 'fusion' on [its own text output ; 5 video tokens] (a [CLS] plus a 2 x 2 patch grid), L = 13 -> fusion/attn_<i> (2, 12, 13, 13),
    fusion/hidden (3, 2, 3, 768): rows {0, last valid text row, first video row}.
The query and key weights are multiplied by QK_GAIN so the maps are far from uniform (the closed-form weights alone give scores of a few
tenths).  case_inputs / case_config / apply_gain need no reference: tests/test_attn_outputs_parity.py builds the same case from them.
The reference is needed only by main(); it never runs on the GPU box.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.det_init import fill_state_dict_, unit_uniform  # noqa: E402

FNAME = "bert_attn_B2.npz"
OVERRIDES = dict(num_hidden_layers=4, fusion_layer=2, vocab_size=2048)
QK_GAIN = 2.0   # scores four times the closed-form weights' (standard deviation about 1): peaked rows, yet a score error of fp16 operands (about 1e-3 of |s|) stays small against the tolerance on p
B, LT, LV, D = 2, 8, 5, 768
LAST_VALID = (LT - 1, LT - 3)          # last valid text row of each caption


def case_inputs():
    """(ids (2, 8) int64, mask (2, 8) int64, video_embeds (2, 5, 768) fp32): closed forms."""
    x = (unit_uniform("attn_golden/ids", B * LT) + 1.0) * 0.5
    ids = torch.from_numpy((110 + np.floor(x * (OVERRIDES["vocab_size"] - 110))).astype(np.int64).reshape(B, LT))
    ids[:, 0] = 101
    mask = torch.ones(B, LT, dtype=torch.long)
    mask[1, LAST_VALID[1] + 1:] = 0
    ids[1, LAST_VALID[1] + 1:] = 0
    ids[0, LAST_VALID[0]] = ids[1, LAST_VALID[1]] = 102
    video = torch.from_numpy((1.5 * unit_uniform("attn_golden/video", B * LV * D)).astype(np.float32).reshape(B, LV, D))
    return ids, mask, video


def apply_gain(bert):
    """det_init weights, then query / key weights and biases times QK_GAIN (same module tree on both sides)."""
    fill_state_dict_(bert)
    with torch.no_grad():
        for layer in bert.encoder.layer:
            for lin in (layer.attention.self.query, layer.attention.self.key):
                lin.weight.mul_(QK_GAIN)
                lin.bias.mul_(QK_GAIN)
    return bert


def hidden_rows(hs, fusion):
    """tuple of (B, L, D) -> (len, B, 2 or 3, D): rows {0, last valid text row[, first video row]} of every entry."""
    out = []
    for h in hs:
        out.append(torch.stack([torch.stack([h[b, 0], h[b, LAST_VALID[b]]] + ([h[b, LT]] if fusion else [])) for b in range(B)]))
    return torch.stack(out)


def main():
    from tests.golden import ref_harness as rh
    _, xbert = rh.import_reference()
    cfg, _ = rh.make_configs(**OVERRIDES)
    m = apply_gain(xbert.BertModel(cfg, add_pooling_layer=False)).eval()
    ids, mask, video = case_inputs()
    g = {}
    with torch.no_grad():
        t = m(ids, attention_mask=mask, return_dict=True, mode="text", output_attentions=True, output_hidden_states=True)
        emb = torch.cat([t.last_hidden_state, video], dim=1)
        att = torch.cat([mask, torch.ones(B, LV, dtype=torch.long)], dim=1)
        f = m(encoder_embeds=emb, attention_mask=att, return_dict=True, mode="fusion", output_attentions=True, output_hidden_states=True)
    for name, o, n_l, L in (("text", t, 2, LT), ("fusion", f, 2, LT + LV)):
        assert len(o.attentions) == n_l and len(o.hidden_states) == n_l + 1
        for i, a in enumerate(o.attentions):
            assert a.shape == (B, 12, L, L)
            g["%s/attn_%d" % (name, i)] = a.numpy().astype(np.float32)
        g["%s/hidden" % name] = hidden_rows(o.hidden_states, name == "fusion").numpy().astype(np.float32)
        g["%s/last_rows" % name] = hidden_rows((o.last_hidden_state,), name == "fusion")[0].numpy().astype(np.float32)
    p = os.path.join(HERE, FNAME)
    np.savez_compressed(p, **g)
    print(FNAME, os.path.getsize(p), {k: v.shape for k, v in g.items()})
    print("peak probability per map:", {k: float(v.max()) for k, v in g.items() if "attn" in k})


if __name__ == "__main__":
    main()
