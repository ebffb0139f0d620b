"""Caption-to-region grounding maps from the fusion encoder's self-attention.

The fusion layers attend over [text ; video tokens] (alpro_models.py:278-281), so the text-query x patch-key block of a fusion layer's softmax
says which regions a caption token reads -- the map the ALBEF line of work visualises.  text_to_patch_attention returns that block alone:
hip.attn_probs is asked for the window (text rows) x (patch keys) of every map, the (L, L) maps are never formed.
"""
import math

import torch


def _layer_indices(layers, n):
    idx = []
    for l in layers:
        i = int(l)
        if not -n <= i < n:
            raise ValueError("text_to_patch_attention: layer %d outside the %d fusion layers" % (i, n))
        idx.append(i % n)
    if not idx:
        raise ValueError("text_to_patch_attention: no layer chosen")
    return idx


@torch.no_grad()
def text_to_patch_attention(model, text_input_ids, text_input_mask, video_embeds, layers=(-1,), reduce_heads="mean"):
    """model: any AlproBaseModel in eval mode; text_input_ids / text_input_mask (B, Lt) and video_embeds (B, 1 + Hg*Wg, D) -- the visual
    encoder's output (model._forward_visual_embeds / encode_video), [CLS] first -- on the device.  Runs the text pass and the fusion pass over
    [text ; video] and returns (B, Lt, Hg, Wg) fp32: for every caption token the probability it puts on each patch token, averaged over the
    heads and over the chosen fusion `layers` (indices into the fusion layers, negative from the end; default: the last one).  The video [CLS]
    key is left out and nothing is renormalised: a token's map sums to the share of its attention that goes to the patches.  Rows of padded
    caption positions are whatever the encoder computes for them (the reference masks keys, not queries)."""
    if model.training:
        raise RuntimeError("text_to_patch_attention inspects a trained model: call model.eval() first (no dropout, no RNG draw)")
    if reduce_heads != "mean":
        raise ValueError("text_to_patch_attention: reduce_heads=%r (only 'mean')" % (reduce_heads,))
    B, Lt = text_input_ids.shape
    Lv = video_embeds.shape[1] if video_embeds.dim() == 3 else 0
    hg = math.isqrt(Lv - 1) if Lv > 1 else 0
    if video_embeds.dim() != 3 or video_embeds.shape[0] != B or hg < 1 or hg * hg != Lv - 1:
        raise ValueError("text_to_patch_attention: video_embeds %s is not (B=%d, 1 + Hg*Wg, D) with a square patch grid" % (tuple(video_embeds.shape), B))
    bert = getattr(model.text_encoder, "bert", model.text_encoder)    # BertForMaskedLM, or the bare BertModel of the QA model
    lo, hi = bert.encoder.layer_range("fusion")
    pick = _layer_indices(layers, hi - lo)
    text_embeds = model._text_embeds(text_input_ids, text_input_mask)
    video_atts = torch.ones((B, Lv), dtype=text_input_mask.dtype, device=text_input_mask.device)
    out = bert(encoder_embeds=torch.cat([text_embeds, video_embeds.to(text_embeds.dtype)], dim=1), attention_mask=torch.cat([text_input_mask, video_atts], dim=1),
               return_dict=True, mode="fusion", output_attentions=True, output_hidden_states=False,
               attn_window=((0, Lt), (Lt + 1, Lt + Lv)))
    acc = None
    for i in pick:   # (B, H, Lt, Hg*Wg) each: head mean, then the layer mean
        m = out.attentions[i].mean(dim=1)
        acc = m if acc is None else acc + m
    return (acc / float(len(pick))).view(B, Lt, hg, hg)
