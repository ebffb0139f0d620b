"""Batch preparation on the device: the per-batch transforms the reference runs on the host / per
sample -- pixel normalisation, BERT-style MLM masking, the random-erase crop that produces the MPM inputs, and the clips'
RandAugment + random square crop -- as batched device ops, so a 300+ pairs/s step is not fed by Python loops over samples,
tokenizer calls and per-frame OpenCV calls.

  ImageNorm                      src/datasets/data_utils.py:437-457   (already a device op there; same in-place semantics)
  mask_batch_text_tokens         src/datasets/data_utils.py:23-70     (80 % [MASK] / 10 % random / 10 % kept, specials and padding never masked)
  random_erase_batch             src/datasets/dataset_pretrain_sparse.py:277-311  (rejection-sampled patch-aligned rectangle per sample)
  TemporalConsistentRandomAugment  src/datasets/randaugment.py:323-361            (N ops per clip, one HIP launch per op stage: alpro_augment_stage)
  sample_square_crops            src/datasets/data_utils.py:310-336  VideoRandomSquareCrop  (offsets on the host, the crop on the kernel's read side)

Randomness comes from torch / numpy generators the caller may pass, so runs are reproducible; the sampling DISTRIBUTIONS are
the reference's, the random streams are not (the reference draws per sample on the host).
"""
import numpy as np
import torch


class ImageNorm:
    """(B, N, 3, H, W) float pixels -> (x / 255 if the data is 0..255 and mean <= 1) - mean) / std, in place."""

    def __init__(self, mean, std, device="cuda"):
        self.mean = torch.tensor(mean, dtype=torch.float32, device=device).view(1, 1, 3, 1, 1)
        self.std = torch.tensor(std, dtype=torch.float32, device=device).view(1, 1, 3, 1, 1)

    def __call__(self, img):
        if torch.max(img) > 1 and self.mean.max() <= 1:
            img.div_(255.)
        return img.sub_(self.mean).div_(self.std)


def mask_batch_text_tokens(inputs, mask_token_id, vocab_size, special_token_ids=(0, 100, 101, 102, 103), pad_token_id=0,
                           mlm_probability=0.15, generator=None):
    """inputs (B, L) int64 on any device, already padded -> (masked inputs, labels) with labels == -100 off the masked positions.
    `special_token_ids` replaces tokenizer.get_special_tokens_mask (bert-base-uncased: [PAD] 0, [UNK] 100, [CLS] 101, [SEP] 102,
    [MASK] 103).  Not in place (the reference overwrites its argument; callers there pass a clone)."""
    inputs = inputs.clone()
    labels = inputs.clone()
    dev = inputs.device
    special = torch.zeros_like(inputs, dtype=torch.bool)
    for t in special_token_ids:
        special |= inputs.eq(t)
    if pad_token_id is not None:
        special |= inputs.eq(pad_token_id)
    prob = torch.full(inputs.shape, mlm_probability, device=dev).masked_fill_(special, 0.0)
    masked = torch.bernoulli(prob, generator=generator).bool()
    labels[~masked] = -100
    replaced = torch.bernoulli(torch.full(inputs.shape, 0.8, device=dev), generator=generator).bool() & masked
    inputs[replaced] = mask_token_id
    rnd = torch.bernoulli(torch.full(inputs.shape, 0.5, device=dev), generator=generator).bool() & masked & ~replaced
    words = torch.randint(vocab_size, inputs.shape, dtype=torch.long, device=dev, generator=generator)
    inputs[rnd] = words[rnd]
    return inputs, labels


def sample_erase_box(img_h, img_w, patch_size, s_l=0.3, s_h=0.5, r_1=0.3, r_2=1 / 0.3, rng=np.random):
    """One patch-aligned rectangle (top, left, h, w) by the reference's rejection sampling."""
    while True:
        s = rng.uniform(s_l, s_h) * img_h * img_w
        r = rng.uniform(r_1, r_2)
        w = int(np.sqrt(s / r))
        h = int(np.sqrt(s * r))
        left = rng.randint(0, img_w)
        top = rng.randint(0, img_h)
        w -= w % patch_size
        h -= h % patch_size
        left -= left % patch_size
        top -= top % patch_size
        if left + w <= img_w and top + h <= img_h:
            return top, left, h, w


def random_erase_batch(visual_inputs, patch_size=16, boxes=None, rng=np.random, **box_kw):
    """visual_inputs (B, T, C, H, W) on the device -> dict(crop_visual_inputs, context_visual_inputs, mpm_mask) as the
    pretraining collator builds them per sample: the crop keeps ONLY the rectangle (zeros elsewhere), the context erases it,
    mpm_mask (B, H/ps, W/ps) is 1 on kept patches and 0 on the rectangle.  One rectangle per sample (host-side sampling of
    4 integers each), applied to the whole batch with two masked selects."""
    B, T, C, H, W = visual_inputs.shape
    if boxes is None:
        boxes = [sample_erase_box(H, W, patch_size, rng=rng, **box_kw) for _ in range(B)]
    dev = visual_inputs.device
    bx = torch.tensor(boxes, dtype=torch.long, device=dev)                      # (B, 4): top, left, h, w
    ys = torch.arange(H, device=dev)[None, :, None]
    xs = torch.arange(W, device=dev)[None, None, :]
    inside = ((ys >= bx[:, 0, None, None]) & (ys < (bx[:, 0] + bx[:, 2])[:, None, None]) &
              (xs >= bx[:, 1, None, None]) & (xs < (bx[:, 1] + bx[:, 3])[:, None, None]))  # (B, H, W)
    m = inside[:, None, None].to(visual_inputs.dtype)
    crop = visual_inputs * m
    context = visual_inputs * (1 - m)
    mpm_mask = 1.0 - torch.nn.functional.avg_pool2d(inside.float()[:, None], kernel_size=patch_size, stride=patch_size)[:, 0]
    return dict(crop_visual_inputs=crop, context_visual_inputs=context, mpm_mask=mpm_mask, boxes=boxes)


def prepare_pretrain_clips(raw, mean, std, patch_size=16, boxes=None, rng=np.random, assume_255=None, augment=None, aug_ops=None,
                           crop_size=None, crop_offsets=None, **box_kw):
    """The whole visual side of a pretraining batch in ONE kernel (alpro_prepare_clips): raw (B, T, 3, H, W) uint8 / float pixels on
    the device -> dict(visual_inputs, crop_visual_inputs, context_visual_inputs, mpm_mask, boxes), identical to what the reference
    assembles from PretrainCollator's random_erase on raw pixels (dataset_pretrain_sparse.py:277-311) followed by ImageNorm on each of
    the three tensors (dataloader.py:104-115): 1 read + 3 writes instead of ~15 elementwise passes.
    assume_255: True / False fixes ImageNorm's data-dependent `torch.max(img) > 1` test (data_utils.py:455) without a device sync;
    None evaluates it (uint8 input is always 0..255).
    augment: a TemporalConsistentRandomAugment -- raw (uint8) first goes through the random square crop (crop_size / crop_offsets, as
    AlproPretrainSparseDataset does at dataset_pretrain_sparse.py:110-111) and the augmenter's op stages, all on the device, and the kernel
    above runs on the uint8 result; the dict then also carries aug_ops and crop_offsets, with which a call can be replayed."""
    from alpro_amd import hip
    replay = None
    if augment is not None:
        if crop_size is not None and int(crop_size) % 4 != 0:
            raise ValueError("prepare_pretrain_clips: crop_size %d is not a multiple of 4, which alpro_prepare_clips needs of the width it reads" % int(crop_size))
        if aug_ops is None:
            aug_ops = augment.sample(raw.shape[0], rng=rng)
        if crop_size is not None and crop_offsets is None:
            crop_offsets = sample_square_crops(raw.shape[0], raw.shape[-2], raw.shape[-1], crop_size, rng=rng)
        raw = augment(raw, ops=aug_ops, crop_size=crop_size, crop_offsets=crop_offsets)
        replay = dict(aug_ops=aug_ops, crop_offsets=crop_offsets)
    elif aug_ops is not None or crop_size is not None or crop_offsets is not None:
        raise ValueError("prepare_pretrain_clips: aug_ops / crop_size / crop_offsets need augment= (TemporalConsistentRandomAugment(p=1.0) crops only)")
    B, T, C, H, W = raw.shape
    if boxes is None:
        boxes = [sample_erase_box(H, W, patch_size, rng=rng, **box_kw) for _ in range(B)]
    if assume_255 is None:
        assume_255 = True if raw.dtype == torch.uint8 else bool(torch.max(raw) > 1)
    scale = (1.0 / 255.0) if (assume_255 and max(mean) <= 1) else 1.0
    bx = torch.tensor(boxes, dtype=torch.int32, device=raw.device)
    vis, crop, ctx = hip.prepare_clips(raw.contiguous(), mean, std, scale, boxes=bx)
    gh, gw = H // patch_size, W // patch_size
    ys = torch.arange(gh, device=raw.device)[None, :, None] * patch_size
    xs = torch.arange(gw, device=raw.device)[None, None, :] * patch_size
    b64 = bx.long()
    inside = ((ys >= b64[:, 0, None, None]) & (ys < (b64[:, 0] + b64[:, 2])[:, None, None]) &
              (xs >= b64[:, 1, None, None]) & (xs < (b64[:, 1] + b64[:, 3])[:, None, None]))
    out = dict(visual_inputs=vis, crop_visual_inputs=crop, context_visual_inputs=ctx, mpm_mask=1.0 - inside.float(), boxes=boxes)
    if replay is not None:
        out.update(replay)
    return out


# ---- TemporalConsistentRandomAugment + VideoRandomSquareCrop on the device (alpro_augment_stage) ----------------------------------------
MAX_LEVEL, TRANSLATE_CONST = 10, 10   # randaugment.py:297-298


def aug_op_args(code, M):
    """The two fp64 arguments alpro_augment_stage takes for op `code` at level M (randaugment.py:219-320): the enhance factor, the
    solarize threshold, the posterize bit count, the translate offset, the shear factor, or (cos, sin) of the rotation angle."""
    from alpro_amd.hip import AUG_OPS as A
    lv = M / MAX_LEVEL
    if code in (A["Brightness"], A["Contrast"], A["Sharpness"], A["Color"]):
        return lv * 1.8 + 0.1, 0.0
    if code == A["Solarize"]:
        return float(int(lv * 256)), 0.0
    if code == A["Posterize"]:
        return float(int(lv * 4)), 0.0
    if code in (A["TranslateX"], A["TranslateY"]):
        return lv * float(TRANSLATE_CONST), 0.0
    if code in (A["ShearX"], A["ShearY"]):
        return lv * 0.3, 0.0
    if code == A["Rotate"]:
        d = np.deg2rad(lv * 30)
        return float(np.cos(d)), float(np.sin(d))
    return 0.0, 0.0


def _randint(rng, high):
    """Uniform integer in [0, high) from the numpy module, a RandomState or a Generator."""
    return int(rng.integers(0, high)) if hasattr(rng, "integers") else int(rng.randint(0, high))


def sample_square_crops(B, H, W, crop_size, rng=np.random):
    """One (top, left) per clip as VideoRandomSquareCrop draws them (data_utils.py:333-334): top uniform in [0, H - crop_size], left
    uniform in [0, W - crop_size], both ends included."""
    crop_size = int(crop_size)
    if crop_size < 1 or crop_size > H or crop_size > W:
        raise ValueError("sample_square_crops: crop_size %d does not fit a %d x %d frame" % (crop_size, H, W))
    return [(_randint(rng, H - crop_size + 1), _randint(rng, W - crop_size + 1)) for _ in range(B)]


class TemporalConsistentRandomAugment:
    """randaugment.py:323-361 on a batch of device clips: per clip N distinct ops drawn from `augs`, each applied (at level M) when a
    uniform draw exceeds p, the same ops on every frame of the clip; one kernel launch per op stage for the whole batch, whatever mix
    of ops the clips drew, uint8 between the stages exactly as the reference chains its per-frame functions.  Deviations: source
    positions of the geometric ops are floating point (OpenCV rounds them to 1/32 pixel), Sharpness clamps where the reference's
    cast is platform-defined, and there is no Equalize (naming it raises; an empty `augs` means the other thirteen ops).
    `tensor_in_tensor_out` is accepted and ignored: input and output are device tensors."""

    def __init__(self, N=2, M=10, p=0.0, tensor_in_tensor_out=True, augs=[]):
        from alpro_amd.hip import AUG_OPS
        self.N, self.M, self.p = int(N), M, p
        self.augs = list(augs) if augs else list(AUG_OPS)
        for name in self.augs:
            if name == "Equalize":
                raise ValueError("TemporalConsistentRandomAugment: 'Equalize' is not built on the device (a per-frame histogram op); take it out of augs")
            if name not in AUG_OPS:
                raise ValueError("TemporalConsistentRandomAugment: unknown op %r (known: %s)" % (name, ", ".join(AUG_OPS)))
        if self.N < 0 or self.N > len(self.augs):
            raise ValueError("TemporalConsistentRandomAugment: N = %d distinct ops cannot be drawn from %d" % (self.N, len(self.augs)))
        self._codes = np.array([AUG_OPS[a] for a in self.augs], dtype=np.int32)
        self._ws = {}   # device -> the intermediate clip buffers and the per-frame sums / tables, reused between calls (stream-ordered)

    def sample(self, B, rng=np.random):
        """(B, N) int32 op codes (hip.AUG_OPS), -1 where the draw skipped the op.  Per clip: N distinct ops, then N uniform draws."""
        ops = np.full((B, self.N), -1, dtype=np.int32)
        for b in range(B):
            picked = self._codes[rng.choice(len(self._codes), self.N, replace=False)]
            apply = np.asarray(rng.random(size=self.N)) > self.p
            ops[b] = np.where(apply, picked, -1)
        return ops

    def _buffer(self, ws, key, shape, dtype, device):
        t = ws.get(key)
        if t is None or t.numel() < int(np.prod(shape)):
            t = ws[key] = torch.empty(int(np.prod(shape)), dtype=dtype, device=device)
        return t[:int(np.prod(shape))].view(shape)

    def __call__(self, clips, ops=None, rng=np.random, crop_size=None, crop_offsets=None):
        """clips (B, T, 3, H, W) contiguous uint8 on the device -> a new (B, T, 3, Hc, Wc) uint8 tensor; ops: what sample() returns
        (default: drawn from rng); crop_size: side of the random square crop applied before the first op (offsets drawn from rng
        unless crop_offsets, a list of (top, left) per clip, is given)."""
        from alpro_amd import hip
        if not isinstance(clips, torch.Tensor) or not clips.is_cuda:
            raise RuntimeError("TemporalConsistentRandomAugment needs a device tensor, got %s (no CPU fallback)" % getattr(clips, "device", type(clips).__name__))
        if clips.dtype != torch.uint8:
            raise RuntimeError("TemporalConsistentRandomAugment needs uint8 pixels, got %s" % clips.dtype)
        if clips.dim() != 5 or clips.shape[2] != 3:
            raise RuntimeError("TemporalConsistentRandomAugment needs (B, T, 3, H, W) clips, got shape %s" % (tuple(clips.shape),))
        if not clips.is_contiguous():
            raise RuntimeError("TemporalConsistentRandomAugment needs a contiguous tensor, got strides %s for shape %s" % (tuple(clips.stride()), tuple(clips.shape)))
        B, T, _, H, W = clips.shape
        dev = clips.device
        ops = self.sample(B, rng=rng) if ops is None else np.asarray(ops, dtype=np.int32)
        if ops.ndim != 2 or ops.shape[0] != B:
            raise ValueError("TemporalConsistentRandomAugment: ops must be (%d, N), got shape %s" % (B, ops.shape))
        if ops.size and (ops.min() < -1 or ops.max() >= len(hip.AUG_OPS)):
            raise ValueError("TemporalConsistentRandomAugment: op codes must lie in -1..%d, got %d..%d" % (len(hip.AUG_OPS) - 1, ops.min(), ops.max()))
        Hc, Wc, crop = H, W, None
        if crop_size is not None:
            Hc = Wc = int(crop_size)
            if Hc < 1 or Hc > H or Wc > W:
                raise ValueError("TemporalConsistentRandomAugment: crop_size %d does not fit the %d x %d frame" % (Hc, H, W))
            if crop_offsets is None:
                crop_offsets = sample_square_crops(B, H, W, Hc, rng=rng)
            off = np.asarray(crop_offsets, dtype=np.int64).reshape(-1, 2)
            if off.shape[0] != B:
                raise ValueError("TemporalConsistentRandomAugment: %d crop offsets for %d clips" % (off.shape[0], B))
            bad = (off[:, 0] < 0) | (off[:, 0] > H - Hc) | (off[:, 1] < 0) | (off[:, 1] > W - Wc)
            if bad.any():
                b = int(np.argmax(bad))
                raise ValueError("TemporalConsistentRandomAugment: crop offset (%d, %d) of clip %d leaves the %d x %d frame with crop_size %d"
                                 % (off[b, 0], off[b, 1], b, H, W, Hc))
            crop = off
        elif crop_offsets is not None:
            raise ValueError("TemporalConsistentRandomAugment: crop_offsets given without crop_size")
        # stages worth a launch: any clip applies an op; the first one launched also carries the crop (a copy stage if none is left)
        stages = [k for k in range(ops.shape[1]) if (ops[:, k] >= 0).any()]
        if not stages:
            ops, stages = np.full((B, 1), -1, dtype=np.int32), [0]
        S = len(stages)
        # every stage's arguments, op codes and the crop offsets in ONE host buffer and one upload: [args fp64 (S, B, 2) | ops int32 (S, B) | crop int32 (B, 2)]
        by_code = {c: aug_op_args(c, self.M) for c in range(-1, len(hip.AUG_OPS))}
        host = np.empty(S * B * 16 + S * B * 4 + B * 8, dtype=np.uint8)
        host[:S * B * 16].view(np.float64).reshape(S, B, 2)[:] = [[by_code[int(c)] for c in ops[:, k]] for k in stages]
        host[S * B * 16:S * B * 20].view(np.int32).reshape(S, B)[:] = ops[:, stages].T
        host[S * B * 20:].view(np.int32).reshape(B, 2)[:] = 0 if crop is None else crop
        devbuf = torch.from_numpy(host).to(dev)
        args_d = devbuf[:S * B * 16].view(torch.float64).view(S, B, 2)
        ops_d = devbuf[S * B * 16:S * B * 20].view(torch.int32).view(S, B)
        crop = None if crop is None else devbuf[S * B * 20:].view(torch.int32).view(B, 2)
        ws = self._ws.setdefault((dev.type, dev.index), {})
        sums = self._buffer(ws, "sums", (B * T, 3), torch.int64, dev)
        tables = self._buffer(ws, "tables", (B * T, 256), torch.uint8, dev)
        contrast = hip.AUG_OPS["Contrast"]
        cur = clips
        for i, k in enumerate(stages):
            last = i == len(stages) - 1
            out_hw = (Hc, Wc) if i == 0 else None
            if (ops[:, k] == contrast).any():
                hip.augment_stats(cur, ops_d[i], args_d[i], sums, tables, crop=crop if i == 0 else None, out_hw=out_hw)
            dst = torch.empty((B, T, 3, Hc, Wc), dtype=torch.uint8, device=dev) if last else self._buffer(ws, "clip%d" % (i & 1), (B, T, 3, Hc, Wc), torch.uint8, dev)
            cur = hip.augment_stage(cur, ops_d[i], args_d[i], tables, dst=dst, crop=crop if i == 0 else None, out_hw=out_hw)
        return cur
