"""Golden vectors for captions long enough to push attention past 256 tokens, from the REFERENCE itself (CPU, fp32, eval).

    python -m tests.golden.make_golden_long          # writes tests/golden/pretrain_T4_L96_B2.npz, retrieval_T2_B2_L320.npz

  * pretrain_T4_L96_B2.npz   AlproForPretrain, 4 frames x 96-token captions: fusion length 96 + 197 = 293 (make_golden.case_pretrain_release
                             at Lt = 96): all four losses, ITM scores, MLM columns, sim_v2t, parameter-gradient norms.
  * retrieval_T2_B2_L320.npz AlproForVideoTextRetrieval, 2 frames x 320-token captions: text encoder at L = 320, fusion at L = 517
                             (several 64-key blocks): ITC / ITM losses and scores, 1-video x B-captions forward_inference, sim_v2t,
                             gradient norms of itm_loss + itc_loss and a few full gradients.
det_batch's padded caption tails keep the key bias in play.  Weights and inputs come from det_init.py closed forms, as in make_golden.py.
Needs the reference; never runs on the GPU box.
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

RET_LONG_GRAD_FULL = ["vision_proj.weight", "text_proj.bias", "itm_head.weight", "itm_head.bias", "temp",
                      "text_encoder.bert.encoder.layer.5.attention.self.value.bias",
                      "text_encoder.bert.encoder.layer.9.attention.self.key.bias",
                      "text_encoder.bert.embeddings.LayerNorm.weight"]


def case_retrieval_long(am, fname, T=2, B=2, Lt=320):
    cfg, venc = rh.make_configs(num_frm=T)
    m = am.AlproForVideoTextRetrieval(cfg, venc)
    fill_state_dict_(m)
    m.eval()
    batch = det_batch(B, T, Lt=Lt, seed_name="retrieval_long", with_mlm=False, with_mpm=False)
    orig = torch.multinomial
    torch.multinomial = mg.argmax_multinomial
    try:
        out = m(batch)
        with torch.no_grad():
            inf = m.forward_inference(dict(visual_inputs=batch["visual_inputs"][:1], text_input_ids=batch["text_input_ids"],
                                           text_input_mask=batch["text_input_mask"]))
    finally:
        torch.multinomial = orig
    g = {k: mg.npf(out[k]) for k in ("itc_loss", "itm_loss", "itm_scores", "itm_labels")}
    g["inf_logits"] = mg.npf(inf["logits"])
    g["inf_itc_scores"] = mg.npf(inf["itc_scores"])
    with torch.no_grad():
        ve = m.visual_encoder.forward_features(batch["visual_inputs"].transpose(1, 2), return_all_tokens=True)
        vf = torch.nn.functional.normalize(m.vision_proj(ve[:, 0, :]), dim=-1)
        te = m.text_encoder.bert(batch["text_input_ids"], attention_mask=batch["text_input_mask"], return_dict=True, mode="text").last_hidden_state
        tf = torch.nn.functional.normalize(m.text_proj(te[:, 0, :]), dim=-1)
        g["sim_v2t"] = mg.npf(vf @ tf.t() / m.temp)
    (out["itm_loss"] + out["itc_loss"]).backward()
    names, norms = [], []
    for n_, p_ in m.named_parameters():
        if p_.grad is not None:
            names.append(n_)
            norms.append(float(p_.grad.norm()))
    g["grad_norm_names"] = np.array(names)
    g["grad_norms"] = np.array(norms, dtype=np.float64)
    pd = dict(m.named_parameters())
    for n_ in RET_LONG_GRAD_FULL:
        assert pd[n_].grad is not None, n_
        g["grad/" + n_] = mg.npf(pd[n_].grad)
    np.savez_compressed(os.path.join(HERE, fname), **g)


def main():
    am, _ = rh.import_reference()
    torch.set_num_threads(8)
    only = set(sys.argv[1:])
    if not only or "pretrain" in only:
        mg.case_pretrain_release(am, "pretrain_T4_L96_B2.npz", T=4, Lt=96)
    if not only or "retrieval" in only:
        case_retrieval_long(am, "retrieval_T2_B2_L320.npz")
    for f in ("pretrain_T4_L96_B2.npz", "retrieval_T2_B2_L320.npz"):
        p = os.path.join(HERE, f)
        if os.path.exists(p):
            print(f, os.path.getsize(p))


if __name__ == "__main__":
    main()
