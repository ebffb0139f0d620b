"""Grounding maps from the encoders' self-attention: caption token -> region (fusion encoder), frame -> region and frame -> frame (visual encoder).

The fusion layers attend over [text ; video tokens] (alpro_models.py:278-281), so the text-query x patch-key block of a fusion layer's softmax
says which regions a caption token reads -- the map the ALBEF line of work visualises.  text_to_patch_attention returns that block alone:
hip.attn_probs is asked for the window (text rows) x (patch keys) of every map, the (L, L) maps are never formed.

The fusion maps are collapsed over time (the fusion encoder sees temporally pooled patch tokens).  Where the visual encoder itself looks, and in
which frame, is in the maps of its divided space-time blocks: frame_patch_attention returns the frame's [CLS] query row of the spatial maps
(again a window: no (1+N, 1+N) map is formed), patch_temporal_attention the (T, T) temporal map of every patch position.

Which patches of which frame, and which frames, made a caption match: frame_patch_gradcam and patch_temporal_gradcam are Grad-CAM
(P * relu(d ITM score / d P)) on those two sets of maps -- the one quantity of ViT explanation that is local in time.

At pixel resolution, per frame: pixel_gradient is d ITM score / d visual_inputs through the fusion layers, the visual encoder and the patch
embedding; text_to_pixel_saliency reduces its channels (input gradient, gradient x input).
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


def text_to_patch_gradcam(model, text_input_ids, text_input_mask, video_embeds, layers=(-1,), target=1, grad_scale=None):
    """Grad-CAM of the ITM score over the patches, per caption token: arguments as text_to_patch_attention; returns (B, Lt, Hg, Wg) fp32,
    P * relu(d score / d P) of the text-query x patch-key block of the chosen fusion `layers`, averaged over the heads, then over the layers,
    with score = itm_head(fusion [CLS])[:, target].sum() (target 1: "match") and P the softmax before dropout.  This is the map the ALBEF line
    of work visualises; the raw attention (text_to_patch_attention) says where a token reads, this one which regions made the caption match.
    The text pass runs without grad, the fusion pass over [text ; video] with a detached copy of video_embeds that requires a gradient, and
    an AttnGradients collector takes the window ((0, Lt), (Lt + 1, Lt + Lv)) from the layers' backward: no (L, L) tensor is formed.

    The model is left untouched: every parameter's requires_grad is False for the duration (no weight-gradient launch, no .grad, no flat
    optimizer buffer is written) and restored afterwards.  The call runs an anchored backward, so it bumps train.BACKWARD_EPOCH: it must not
    sit between an optimizer's synchronize() and step().
    grad_scale: fp16 operands need a scaled backward (activation gradients underflow otherwise): the score is multiplied by grad_scale, the
    kernel divides G by it; a power of two, so the rescale is exact.  None: the initial scale of alpro_amd.amp.LossScaler under fp16, 1 under
    bf16 / fp32.  A non-finite map raises (fp16: lower grad_scale); there is no retry."""
    from alpro_amd import config as rt
    from alpro_amd.modeling.alpro_models import _linear32
    from alpro_amd.modeling.xbert import AttnGradients
    what = "text_to_patch_gradcam"
    if model.training:
        raise RuntimeError("%s inspects a trained model: call model.eval() first (no dropout, no RNG draw)" % what)
    B, Lt = text_input_ids.shape
    Lv = video_embeds.shape[1] if video_embeds.dim() == 3 else 0
    hg = math.isqrt(Lv - 1) if Lv > 1 else 0
    if video_embeds.dim() != 3 or video_embeds.shape[0] != B or hg < 1 or hg * hg != Lv - 1:
        raise ValueError("%s: video_embeds %s is not (B=%d, 1 + Hg*Wg, D) with a square patch grid" % (what, tuple(video_embeds.shape), B))
    grad_scale = _power_of_two_scale(grad_scale, what)
    bert = getattr(model.text_encoder, "bert", model.text_encoder)    # BertForMaskedLM, or the bare BertModel of the QA model
    lo, hi = bert.encoder.layer_range("fusion")
    pick = _layer_indices(layers, hi - lo)
    collector = AttnGradients(layers=pick, window=((0, Lt), (Lt + 1, Lt + Lv)), want=("cam",), grad_scale=grad_scale)
    flags = [(p, p.requires_grad) for p in model.parameters()]
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        with torch.no_grad():
            text_embeds = model._text_embeds(text_input_ids, text_input_mask)
        video = video_embeds.detach().to(text_embeds.dtype).clone().requires_grad_(True)
        video_atts = torch.ones((B, Lv), dtype=text_input_mask.dtype, device=text_input_mask.device)
        with torch.enable_grad():
            out = bert(encoder_embeds=torch.cat([text_embeds, video], dim=1), attention_mask=torch.cat([text_input_mask, video_atts], dim=1),
                       return_dict=True, mode="fusion", attn_grads=collector).last_hidden_state
            score = _linear32(out[:, 0, :], model.itm_head)[:, int(target)].sum() * grad_scale
            with rt.loss_scaling(collector):   # (marks the backward as scaled: config.check_backward_precision)
                score.backward()
    finally:
        for p, f in flags:
            p.requires_grad_(f)
    acc = None
    for i in pick:   # (B, H, Lt, Hg*Wg) each: head mean, then the layer mean
        m = collector.cams[i].mean(dim=1)
        acc = m if acc is None else acc + m
    res = (acc / float(len(pick))).view(B, Lt, hg, hg)
    if not bool(torch.isfinite(res).all()):
        raise RuntimeError("%s: the map is not finite at grad_scale=%g -- the scaled backward left fp16's range; pass a smaller power of two as grad_scale"
                           % (what, grad_scale))
    return res


def _power_of_two_scale(grad_scale, what):
    from alpro_amd import config as rt
    if grad_scale is None:
        from alpro_amd.amp import LossScaler
        grad_scale = LossScaler()._init if rt.compute_dtype() == torch.float16 else 1.0
    grad_scale = float(grad_scale)
    if not grad_scale > 0 or math.frexp(grad_scale)[0] != 0.5:
        raise ValueError("%s: grad_scale=%r is not a positive power of two (the rescale of the gradient must be exact)" % (what, grad_scale))
    return grad_scale


def pixel_gradient(model, text_input_ids, text_input_mask, visual_inputs, target=1, grad_scale=None, _what="pixel_gradient"):
    """d score / d visual_inputs at pixel resolution: model any AlproBaseModel with an itm_head, in eval mode; text_input_ids / text_input_mask
    (B, Lt) and visual_inputs (B, T, C, H, W), as the models take them, on the device.  Returns (B, T, C, H, W) fp32, contiguous, with
    score = itm_head(fusion [CLS])[:, target].sum() over the pairs (caption b, clip b) (target 1: "match").  Where text_to_patch_gradcam gives
    one patch grid per caption token, averaged over the frames, this says which pixels of which frame made the caption match; it is what
    gradient x input, SmoothGrad, integrated gradients and adversarial-robustness evaluations start from.
    The text pass runs without grad; the visual pass and the fusion pass run with grad on a detached copy of the clip, and the hand-written
    backward goes through the fusion layers, the twelve divided space-time blocks and the patch embedding (alpro_unpatchify) to the pixels.

    The model is left untouched, exactly as by text_to_patch_gradcam: every parameter's requires_grad is False for the duration (no
    weight-gradient launch, no .grad, no flat optimizer buffer is written) and restored afterwards; the call bumps train.BACKWARD_EPOCH.
    grad_scale: the score is multiplied by it and the gradient divided by it afterwards; a positive power of two, so the rescale is exact.
    None: the initial scale of alpro_amd.amp.LossScaler under fp16 (whose backward must be scaled), 1 under bf16 / fp32.  A non-finite result
    raises (fp16: lower grad_scale); there is no retry."""
    from alpro_amd import config as rt
    from alpro_amd.modeling.alpro_models import _linear32
    what = _what
    if model.training:
        raise RuntimeError("%s inspects a trained model: call model.eval() first (no dropout, no drop-path, no RNG draw)" % what)
    _grid(visual_inputs, what)
    if text_input_ids.dim() != 2 or text_input_ids.shape != text_input_mask.shape or text_input_ids.shape[0] != visual_inputs.shape[0]:
        raise ValueError("%s: text_input_ids %s / text_input_mask %s are not (B=%d, Lt), one caption per clip of visual_inputs %s"
                         % (what, tuple(text_input_ids.shape), tuple(text_input_mask.shape), visual_inputs.shape[0], tuple(visual_inputs.shape)))
    grad_scale = _power_of_two_scale(grad_scale, what)
    B = visual_inputs.shape[0]
    flags = [(p, p.requires_grad) for p in model.parameters()]
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        with torch.no_grad():
            text_embeds = model._text_embeds(text_input_ids, text_input_mask)
        clip = visual_inputs.detach().float().clone().requires_grad_(True)
        with torch.enable_grad():
            video = model.visual_encoder.forward_features(clip.transpose(1, 2), return_all_tokens=True)
            video_atts = torch.ones((B, video.shape[1]), dtype=text_input_mask.dtype, device=text_input_mask.device)
            out = model._fusion(torch.cat([text_embeds, video.to(text_embeds.dtype)], dim=1), torch.cat([text_input_mask, video_atts], dim=1))
            score = _linear32(out[:, 0, :], model.itm_head)[:, int(target)].sum() * grad_scale
            with rt.loss_scaling(clip):   # (marks the backward as scaled: config.check_backward_precision)
                score.backward()
    finally:
        for p, f in flags:
            p.requires_grad_(f)
    res = clip.grad
    if grad_scale != 1.0:
        res = res / grad_scale
    if not bool(torch.isfinite(res).all()):
        raise RuntimeError("%s: the gradient is not finite at grad_scale=%g -- the scaled backward left fp16's range; pass a smaller power of two as grad_scale"
                           % (what, grad_scale))
    return res


SALIENCY_METHODS = ("grad_x_input", "grad")


def text_to_pixel_saliency(model, text_input_ids, text_input_mask, visual_inputs, target=1, grad_scale=None, method="grad_x_input"):
    """Pixel saliency of the ITM score: arguments as pixel_gradient; returns (B, T, H, W) fp32, the channels of g = pixel_gradient(...) reduced by
    `method`: "grad" -> max_c |g| (input-gradient saliency), "grad_x_input" -> sum_c g * x (gradient x input, signed: the first-order share of
    each pixel in the score)."""
    if method not in SALIENCY_METHODS:
        raise ValueError("text_to_pixel_saliency: method=%r (one of %s)" % (method, ", ".join(repr(m) for m in SALIENCY_METHODS)))
    g = pixel_gradient(model, text_input_ids, text_input_mask, visual_inputs, target=target, grad_scale=grad_scale, _what="text_to_pixel_saliency")
    if method == "grad":
        return g.abs().amax(dim=2)
    return (g * visual_inputs.detach().float()).sum(dim=2)


def _visual_encoder(encoder, what):
    enc = getattr(encoder, "visual_encoder", encoder)    # an AlproBaseModel, or the TimeSformer itself
    if enc.training:
        raise RuntimeError("%s inspects a trained model: call model.eval() first (no dropout, no drop-path, no RNG draw)" % what)
    return enc


def _grid(visual_inputs, what):
    if visual_inputs.dim() != 5 or visual_inputs.shape[3] % 16 or visual_inputs.shape[4] % 16:
        raise ValueError("%s: visual_inputs %s is not (B, T, C, H, W) with H and W multiples of the 16-pixel patch" % (what, tuple(visual_inputs.shape)))
    B, T, _, H, W = visual_inputs.shape
    return B, T, H // 16, W // 16


def _block_mean(maps, layers, what):
    pick = []
    for l in layers:
        i = int(l)
        if not -len(maps) <= i < len(maps):
            raise ValueError("%s: layer %d outside the %d blocks" % (what, i, len(maps)))
        pick.append(i % len(maps))
    if not pick:
        raise ValueError("%s: no layer chosen" % what)
    return pick


@torch.no_grad()
def frame_patch_attention(encoder, visual_inputs, layers=(-1,), reduce_heads="mean"):
    """encoder: a TimeSformer, or any AlproBaseModel (its visual_encoder is used), in eval mode; visual_inputs (B, T, C, H, W) on the device, as
    the models take them.  Returns (B, T, Hg, Wg) fp32: the probability the frame's [CLS] query puts on each patch of ITS frame in the spatial
    attention, averaged over the heads and over the chosen blocks `layers` (negative: from the end; default: the last block).  Only the window
    ((0, 1), (1, 1 + N)) of the chosen blocks' spatial maps is formed.  The [CLS] key is left out and nothing is renormalised: a frame's map
    sums to the share of the [CLS] query's attention that goes to the patches."""
    what = "frame_patch_attention"
    enc = _visual_encoder(encoder, what)
    if reduce_heads != "mean":
        raise ValueError("%s: reduce_heads=%r (only 'mean')" % (what, reduce_heads))
    B, T, hg, wg = _grid(visual_inputs, what)
    depth = len(enc.model.blocks)
    pick = sorted(set(_block_mean(range(depth), layers, what)))
    out = enc.forward_features(visual_inputs.transpose(1, 2), output_attentions=True, attn_layers=pick, attn_window=((0, 1), (1, 1 + hg * wg)))
    acc = None
    for l in layers:   # (B*T, H, 1, N) each, in block order: head mean, then the layer mean
        m = out.spatial_attentions[pick.index(int(l) % depth)].mean(dim=1)
        acc = m if acc is None else acc + m
    return (acc / float(len(layers))).view(B, T, hg, wg)


@torch.no_grad()
def patch_temporal_attention(encoder, visual_inputs, layers=(-1,)):
    """As frame_patch_attention, for the temporal half: returns (B, Hg, Wg, T, T) fp32, the temporal attention map (query frame, key frame) of every
    patch position, averaged over the heads and over the chosen blocks."""
    what = "patch_temporal_attention"
    enc = _visual_encoder(encoder, what)
    B, T, hg, wg = _grid(visual_inputs, what)
    depth = len(enc.model.blocks)
    pick = sorted(set(_block_mean(range(depth), layers, what)))
    # (the spatial maps come with the flag: keep them to one element per frame and head)
    out = enc.forward_features(visual_inputs.transpose(1, 2), output_attentions=True, attn_layers=pick, attn_window=((0, 1), (0, 1)))
    acc = None
    for l in layers:   # (B*N, H, T, T) each
        m = out.temporal_attentions[pick.index(int(l) % depth)].mean(dim=1)
        acc = m if acc is None else acc + m
    return (acc / float(len(layers))).view(B, hg, wg, T, T)


def _vit_gradcam(model, text_input_ids, text_input_mask, visual_inputs, layers, target, grad_scale, what, spatial):
    """The shared body of frame_patch_gradcam (spatial) and patch_temporal_gradcam: -> (B, T, Hg, Wg, list of the chosen blocks' CAM head means)."""
    from alpro_amd import config as rt
    from alpro_amd.modeling.alpro_models import _linear32
    from alpro_amd.modeling.timesformer.vit import VitAttnGradients
    if model.training:
        raise RuntimeError("%s inspects a trained model: call model.eval() first (no dropout, no drop-path, no RNG draw)" % what)
    B, T, hg, wg = _grid(visual_inputs, what)
    if text_input_ids.dim() != 2 or text_input_ids.shape != text_input_mask.shape or text_input_ids.shape[0] != B:
        raise ValueError("%s: text_input_ids %s / text_input_mask %s are not (B=%d, Lt), one caption per clip of visual_inputs %s"
                         % (what, tuple(text_input_ids.shape), tuple(text_input_mask.shape), B, tuple(visual_inputs.shape)))
    grad_scale = _power_of_two_scale(grad_scale, what)
    depth = len(model.visual_encoder.model.blocks)
    pick = _block_mean(range(depth), layers, what)
    collector = VitAttnGradients(layers=pick, want=("cam",), spatial=spatial, temporal=not spatial,
                                 spatial_window=((0, 1), (1, 1 + hg * wg)) if spatial else None, grad_scale=grad_scale)
    flags = [(p, p.requires_grad) for p in model.parameters()]
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        with torch.no_grad():
            text_embeds = model._text_embeds(text_input_ids, text_input_mask)
        clip = visual_inputs.detach().float()   # (needs no gradient: the backward stops at the first chosen block)
        with torch.enable_grad():
            video = model.visual_encoder.forward_features(clip.transpose(1, 2), return_all_tokens=True, attn_grads=collector)
            video_atts = torch.ones((B, video.shape[1]), dtype=text_input_mask.dtype, device=text_input_mask.device)
            out = model._fusion(torch.cat([text_embeds, video.to(text_embeds.dtype)], dim=1), torch.cat([text_input_mask, video_atts], dim=1))
            score = _linear32(out[:, 0, :], model.itm_head)[:, int(target)].sum() * grad_scale
            with rt.loss_scaling(collector):   # (marks the backward as scaled: config.check_backward_precision)
                score.backward()
    finally:
        for p, f in flags:
            p.requires_grad_(f)
    cams = collector.spatial_cams if spatial else collector.temporal_cams
    acc = None
    for i in pick:   # head mean, then the layer mean
        m = cams[i].mean(dim=1)
        acc = m if acc is None else acc + m
    res = acc / float(len(pick))
    if not bool(torch.isfinite(res).all()):
        raise RuntimeError("%s: the map is not finite at grad_scale=%g -- the scaled backward left fp16's range; pass a smaller power of two as grad_scale"
                           % (what, grad_scale))
    return B, T, hg, wg, res


def frame_patch_gradcam(model, text_input_ids, text_input_mask, visual_inputs, layers=(-1,), target=1, grad_scale=None):
    """Grad-CAM of the ITM score over the patches of every frame: arguments as pixel_gradient, plus `layers` (blocks of the visual encoder,
    negative from the end; default: the last one).  Returns (B, T, Hg, Wg) fp32: P * relu(d score / d P) of the frame's [CLS] query against
    the patches of ITS frame in the spatial attention -- the window ((0, 1), (1, 1 + N)), no (1+N, 1+N) tensor is formed --, averaged over the
    heads, then over the chosen blocks, with score = itm_head(fusion [CLS])[:, target].sum() (target 1: "match") and P the softmax before
    dropout.  Where frame_patch_attention says where a frame's [CLS] reads, this says which patches of which frame made the caption match;
    text_to_patch_gradcam's map is the same question averaged over the frames.  With precise [CLS] rows P and G of this query row are the
    16-bit graph's.
    The text pass runs without grad; the visual and the fusion pass run with grad, but the clip needs no gradient: the backward goes through the
    fusion layers and the visual blocks down to the first chosen one and stops there.  The model is left untouched, exactly as by
    text_to_patch_gradcam (requires_grad False for the duration and restored, no .grad written, train.BACKWARD_EPOCH bumped); grad_scale as there:
    a positive power of two, None = the initial scale of alpro_amd.amp.LossScaler under fp16, 1 otherwise; a non-finite map raises, no retry."""
    B, T, hg, wg, res = _vit_gradcam(model, text_input_ids, text_input_mask, visual_inputs, layers, target, grad_scale, "frame_patch_gradcam", True)
    return res.view(B, T, hg, wg)


def patch_temporal_gradcam(model, text_input_ids, text_input_mask, visual_inputs, layers=(-1,), target=1, grad_scale=None):
    """As frame_patch_gradcam, for the temporal half: returns (B, Hg, Wg, T, T) fp32, P * relu(d score / d P) of the temporal attention map
    (query frame, key frame) of every patch position, averaged over the heads, then over the chosen blocks: which frames made the caption match,
    and through which other frames."""
    B, T, hg, wg, res = _vit_gradcam(model, text_input_ids, text_input_mask, visual_inputs, layers, target, grad_scale, "patch_temporal_gradcam", False)
    return res.view(B, hg, wg, T, T)
