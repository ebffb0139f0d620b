"""Golden vectors at frame counts that do not divide 32 (temporal attention on the windowed kernels), from the REFERENCE itself (CPU, fp32).

    python -m tests.golden.make_golden_frames        # writes tests/golden/retrieval_T12_B2.npz, pretrain_T6_B2.npz, vit_T48_B1.npz

  * retrieval_T12_B2.npz  AlproForVideoTextRetrieval at 12 frames: ITC / ITM losses and scores, 1-video x B-captions forward_inference,
                          sim_v2t, gradient norms of itm_loss + itc_loss and a few full gradients (time_embed, a temporal-attention qkv bias).
  * pretrain_T6_B2.npz    AlproForPretrain at the released geometry (make_golden.case_pretrain_release) with 6 frames -- the prompter pass
                          runs at 6 frames too: all four losses, ITM scores, MLM columns, sim_v2t, parameter-gradient norms.
  * vit_T48_B1.npz        the visual encoder alone at 48 frames: pooled ([CLS]) features, a row subsample, row norms and row sums of
                          video_embeds, gradient norms of the fixed scalar sum(video_embeds * R), R = det_init.unit_uniform("frames/vit_probe").
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
from tests.golden.det_init import det_batch, fill_state_dict_, unit_uniform  # noqa: E402

RET_FRAMES_GRAD_FULL = ["text_proj.bias", "itm_head.weight", "itm_head.bias", "temp", "visual_encoder.model.time_embed",
                        "visual_encoder.model.blocks.0.temporal_attn.qkv.bias", "visual_encoder.model.blocks.11.temporal_attn.qkv.bias"]
VIT_ROWS = [0, 1, 100, 196]


def vit_probe(T_embed_rows=197):
    return torch.from_numpy(unit_uniform("frames/vit_probe", T_embed_rows * 768).astype(np.float32)).view(1, T_embed_rows, 768)


def _grad_norms(m, g):
    names, norms = [], []
    for n_, p_ in m.named_parameters():
        if p_.grad is not None:
            names.append(n_)
            norms.append(float(p_.grad.norm()))
    g["grad_norm_names"] = np.array(names)
    g["grad_norms"] = np.array(norms, dtype=np.float64)


def case_retrieval_frames_ft(am, fname, T=12, B=2):
    cfg, venc = rh.make_configs(num_frm=T)
    m = am.AlproForVideoTextRetrieval(cfg, venc)
    fill_state_dict_(m)
    m.eval()
    batch = det_batch(B, T, seed_name="retrieval_frames_T%d" % T, with_mlm=False, with_mpm=False)
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
        mg.summarize_embeds("video_embeds", ve, VIT_ROWS, g)
    (out["itm_loss"] + out["itc_loss"]).backward()
    _grad_norms(m, g)
    pd = dict(m.named_parameters())
    for n_ in RET_FRAMES_GRAD_FULL:
        assert pd[n_].grad is not None, n_
        g["grad/" + n_] = mg.npf(pd[n_].grad)
    np.savez_compressed(os.path.join(HERE, fname), **g)


def case_vit_frames(am, fname, T=48, B=1):
    cfg, venc = rh.make_configs(num_frm=T)
    m = am.AlproForVideoTextRetrieval(cfg, venc)
    fill_state_dict_(m)
    m.eval()
    enc = m.visual_encoder
    batch = det_batch(B, T, seed_name="vit_frames_T%d" % T, with_mlm=False, with_mpm=False)
    ve = enc.forward_features(batch["visual_inputs"].transpose(1, 2), return_all_tokens=True)
    g = {"pooled": mg.npf(ve[:, 0])}
    mg.summarize_embeds("video_embeds", ve, VIT_ROWS, g)
    (ve * vit_probe(ve.shape[1])).sum().backward()
    _grad_norms(enc, g)
    g["grad/model.time_embed"] = mg.npf(enc.model.time_embed.grad)
    np.savez_compressed(os.path.join(HERE, fname), **g)


def main():
    am, _ = rh.import_reference()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    only = set(sys.argv[1:])
    if not only or "retrieval" in only:
        case_retrieval_frames_ft(am, "retrieval_T12_B2.npz")
    if not only or "pretrain" in only:
        mg.case_pretrain_release(am, "pretrain_T6_B2.npz", T=6)
    if not only or "vit" in only:
        case_vit_frames(am, "vit_T48_B1.npz")
    for f in ("retrieval_T12_B2.npz", "pretrain_T6_B2.npz", "vit_T48_B1.npz"):
        p = os.path.join(HERE, f)
        if os.path.exists(p):
            print(f, os.path.getsize(p))


if __name__ == "__main__":
    main()
