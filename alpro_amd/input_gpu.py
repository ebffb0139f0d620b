"""Batch preparation on the device: the per-batch transforms the reference runs on the host / per
sample -- pixel normalisation, BERT-style MLM masking, the random-erase crop that produces the MPM inputs, and the clips'
RandAugment + random square crop -- as batched device ops, so a 300+ pairs/s step is not fed by Python loops over samples,
tokenizer calls and per-frame OpenCV calls.

  ImageNorm                      src/datasets/data_utils.py:437-457   (already a device op there; same in-place semantics)
  mask_batch_text_tokens         src/datasets/data_utils.py:23-70     (80 % [MASK] / 10 % random / 10 % kept, specials and padding never masked)
  random_erase_batch             src/datasets/dataset_pretrain_sparse.py:277-311  (rejection-sampled patch-aligned rectangle per sample)
  TemporalConsistentRandomAugment  src/datasets/randaugment.py:323-361            (N ops per clip, one HIP launch per op stage: alpro_augment_stage)
  sample_square_crops            src/datasets/data_utils.py:310-336  VideoRandomSquareCrop  (offsets on the host, the crop on the kernel's read side)
  prepare_pretrain_images        src/datasets/dataset_pretrain_sparse.py:125-193  the image-text stream: RandomResizedCrop + flip (alpro_resized_crop,
                                 PIL's 8-bit bicubic bit for bit), RandomAugment on the same op stages, the image repeated to num_frm frames

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


def video_ids(names, device="cuda"):
    """List of video names (the collator's vid_id per pair; None: a pair without one, e.g. an image-text pair) -> (B,) int64 for the batch key
    `video_ids`: the first 8 bytes of blake2b(UTF-8 name), big-endian, masked to 63 bits; None -> -1 ("no id": the pair matches only itself).
    The same on every rank and in every process (Python's hash() is salted per process), so ids gathered across ranks compare."""
    import hashlib
    vals = [-1 if n is None else int.from_bytes(hashlib.blake2b(str(n).encode("utf-8"), digest_size=8).digest(), "big") & ((1 << 63) - 1)
            for n in names]
    return torch.tensor(vals, dtype=torch.int64).to(device)


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


class _StageAugment:
    """What the two augmenters share: the op list and its refusals, and __call__, which runs the ops sample() drew (or the caller gave) as
    one alpro_augment_stage launch per op stage.  Messages carry the name of the class in use."""

    def _set_augs(self, augs):
        from alpro_amd.hip import AUG_OPS
        who = type(self).__name__
        self.augs = list(augs) if augs else list(AUG_OPS)
        for name in self.augs:
            if name == "Equalize":
                raise ValueError("%s: 'Equalize' is not built on the device (a per-frame histogram op); take it out of augs" % who)
            if name not in AUG_OPS:
                raise ValueError("%s: unknown op %r (known: %s)" % (who, name, ", ".join(AUG_OPS)))
        self._codes = np.array([AUG_OPS[a] for a in self.augs], dtype=np.int32)
        self._ws = {}   # device -> the intermediate clip buffers and the per-frame sums / tables, reused between calls (stream-ordered)

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
        who = type(self).__name__
        if not isinstance(clips, torch.Tensor) or not clips.is_cuda:
            raise RuntimeError("%s needs a device tensor, got %s (no CPU fallback)" % (who, getattr(clips, "device", type(clips).__name__)))
        if clips.dtype != torch.uint8:
            raise RuntimeError("%s needs uint8 pixels, got %s" % (who, clips.dtype))
        if clips.dim() != 5 or clips.shape[2] != 3:
            raise RuntimeError("%s needs (B, T, 3, H, W) clips, got shape %s" % (who, tuple(clips.shape)))
        if not clips.is_contiguous():
            raise RuntimeError("%s needs a contiguous tensor, got strides %s for shape %s" % (who, tuple(clips.stride()), tuple(clips.shape)))
        B, T, _, H, W = clips.shape
        dev = clips.device
        ops = self.sample(B, rng=rng) if ops is None else np.asarray(ops, dtype=np.int32)
        if ops.ndim != 2 or ops.shape[0] != B:
            raise ValueError("%s: ops must be (%d, N), got shape %s" % (who, B, ops.shape))
        if ops.size and (ops.min() < -1 or ops.max() >= len(hip.AUG_OPS)):
            raise ValueError("%s: op codes must lie in -1..%d, got %d..%d" % (who, len(hip.AUG_OPS) - 1, ops.min(), ops.max()))
        Hc, Wc, crop = H, W, None
        if crop_size is not None:
            Hc = Wc = int(crop_size)
            if Hc < 1 or Hc > H or Wc > W:
                raise ValueError("%s: crop_size %d does not fit the %d x %d frame" % (who, Hc, H, W))
            if crop_offsets is None:
                crop_offsets = sample_square_crops(B, H, W, Hc, rng=rng)
            off = np.asarray(crop_offsets, dtype=np.int64).reshape(-1, 2)
            if off.shape[0] != B:
                raise ValueError("%s: %d crop offsets for %d clips" % (who, off.shape[0], B))
            bad = (off[:, 0] < 0) | (off[:, 0] > H - Hc) | (off[:, 1] < 0) | (off[:, 1] > W - Wc)
            if bad.any():
                b = int(np.argmax(bad))
                raise ValueError("%s: crop offset (%d, %d) of clip %d leaves the %d x %d frame with crop_size %d" % (who, off[b, 0], off[b, 1], b, H, W, Hc))
            crop = off
        elif crop_offsets is not None:
            raise ValueError("%s: crop_offsets given without crop_size" % who)
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


class TemporalConsistentRandomAugment(_StageAugment):
    """randaugment.py:323-361 on a batch of device clips: per clip N distinct ops drawn from `augs`, each applied (at level M) when a
    uniform draw exceeds p, the same ops on every frame of the clip; one kernel launch per op stage for the whole batch, whatever mix
    of ops the clips drew, uint8 between the stages exactly as the reference chains its per-frame functions.  Deviations: source
    positions of the geometric ops are floating point (OpenCV rounds them to 1/32 pixel), Sharpness clamps where the reference's
    cast is platform-defined, and there is no Equalize (naming it raises; an empty `augs` means the other thirteen ops).
    `tensor_in_tensor_out` is accepted and ignored: input and output are device tensors."""

    def __init__(self, N=2, M=10, p=0.0, tensor_in_tensor_out=True, augs=[]):
        self.N, self.M, self.p = int(N), M, p
        self._set_augs(augs)
        if self.N < 0 or self.N > len(self.augs):
            raise ValueError("TemporalConsistentRandomAugment: N = %d distinct ops cannot be drawn from %d" % (self.N, len(self.augs)))

    def sample(self, B, rng=np.random):
        """(B, N) int32 op codes (hip.AUG_OPS), -1 where the draw skipped the op.  Per clip: N distinct ops, then N uniform draws."""
        ops = np.full((B, self.N), -1, dtype=np.int32)
        for b in range(B):
            picked = self._codes[rng.choice(len(self._codes), self.N, replace=False)]
            apply = np.asarray(rng.random(size=self.N)) > self.p
            ops[b] = np.where(apply, picked, -1)
        return ops


class RandomAugment(_StageAugment):
    """randaugment.py:363-387, the image form, on a batch of device images (B, T, 3, H, W) -- T = 1 for an image, any T gets the image's ops
    on every frame: per image N ops drawn from `augs` WITH replacement (the same op may come twice), each applied at level M with probability
    0.5 (the reference skips an op when its uniform draw is > 0.5).  The stages, their deviations and the refusal of Equalize are those of
    TemporalConsistentRandomAugment.  `isPIL` is accepted and ignored: input and output are device tensors."""

    PROB = 0.5   # randaugment.py:376

    def __init__(self, N=2, M=10, isPIL=False, augs=[]):
        self.N, self.M = int(N), M
        self._set_augs(augs)
        if self.N < 0:
            raise ValueError("RandomAugment: N = %d ops cannot be drawn" % self.N)

    def sample(self, B, rng=np.random):
        """(B, N) int32 op codes (hip.AUG_OPS), -1 where the draw skipped the op.  Per image: N ops with replacement, then one uniform draw each."""
        ops = np.full((B, self.N), -1, dtype=np.int32)
        for b in range(B):
            picked = self._codes[rng.choice(len(self._codes), self.N)]
            apply = np.asarray(rng.random(size=self.N)) <= self.PROB
            ops[b] = np.where(apply, picked, -1)
        return ops


# ---- RandomResizedCrop + RandomHorizontalFlip on the device (alpro_resized_crop) -------------------------------------------------------------
PRECISION_BITS = 22   # PIL's Resample.c: 32 - 8 - 2


def resample_ksize(in_size, out_size):
    """Tap slots per output index of PIL's bicubic resampling of in_size pixels to out_size: 2 * ceil(support) + 1, support = 2 * max(in / out, 1)."""
    return int(np.ceil(2.0 * max(in_size / out_size, 1.0))) * 2 + 1


def _resample_coeffs(in_sizes, out_size, ktaps):
    """resample_coeffs for several input sizes at once: in_sizes (n) -> (bounds (n, out, 2), k (n, out, ktaps)), ktaps >= every size's tap slots.
    Elementwise over sizes, output indices and taps: each number goes through PIL's operations in PIL's order (slots past a size's own
    tap count hold zero weights, which change neither its sum nor its coefficients)."""
    size = np.asarray(in_sizes, dtype=np.int64)[:, None]                      # (n, 1)
    scale = size / np.float64(out_size)
    fs = np.maximum(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64)[None, :] + 0.5) * scale    # (n, out)
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    n = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), size) - xmin
    x = np.arange(ktaps, dtype=np.int64)[None, None, :]
    t = np.abs(((x + xmin[:, :, None]).astype(np.float64) - center[:, :, None] + 0.5) * ss[:, :, None])
    a = -0.5
    w = np.where(t < 1.0, ((a + 2.0) * t - (a + 3.0)) * t * t + 1, np.where(t < 2.0, (((t - 5) * t + 8) * t - 4) * a, 0.0))
    w = np.where(x < n[:, :, None], w, 0.0)
    ww = np.cumsum(w, axis=2)[:, :, -1:]   # a running sum: index order, as PIL adds them (the zeros past the count change nothing)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    k = np.where(w < 0, np.trunc(-0.5 + w * (1 << PRECISION_BITS)), np.trunc(0.5 + w * (1 << PRECISION_BITS))).astype(np.int32)
    return np.stack([xmin, n], axis=2).astype(np.int32), k


def resample_coeffs(in_size, out_size):
    """PIL's 8-bit bicubic (a = -0.5) coefficients for resizing in_size pixels to out_size (Resample.c precompute_coeffs + normalize_coeffs_8bpc)
    -> (bounds (out, 2) int32 {first tap, tap count}, k (out, ksize) int32, zero past the count), with which
    out[xx] = clip8((2^21 + sum_x k[xx, x] * pix[first + x]) >> 22).  fp64 throughout, every operation in PIL's order (the weights of an output
    index are summed in index order); vectorised over the output indices and the taps only."""
    bounds, k = _resample_coeffs([int(in_size)], int(out_size), resample_ksize(in_size, out_size))
    return bounds[0], k[0]


def resample_table(sizes, boxes, flips, out_size):
    """What alpro_resized_crop reads beside the pixels, as ONE host buffer (uint8) for one upload: [meta int64 (B, 8) {byte offset, H, W, top,
    left, h, w, flip} | coef int32 (B, 2, out_size, 2 + ktaps) {first tap, count, k[0..ktaps)} for the horizontal (axis 0, over w) and the
    vertical (axis 1, over h) pass], ktaps the batch maximum of the tap slots, shorter rows zero-padded.  -> (buffer, max h, ktaps).  Images lie
    back to back in the packed buffer in the order of `sizes`."""
    B, S = len(sizes), int(out_size)
    sz, bx = np.asarray(sizes, dtype=np.int64).reshape(B, 2), np.asarray(boxes, dtype=np.int64).reshape(B, 4)
    ktaps = resample_ksize(int(bx[:, 2:].max()), S)
    host = np.zeros(B * 64 + B * 2 * S * (2 + ktaps) * 4, dtype=np.uint8)
    meta = host[:B * 64].view(np.int64).reshape(B, 8)
    coef = host[B * 64:].view(np.int32).reshape(B, 2, S, 2 + ktaps)
    nbytes = sz[:, 0] * sz[:, 1] * 3
    meta[:, 0] = np.cumsum(nbytes) - nbytes
    meta[:, 1:3], meta[:, 3:7] = sz, bx
    meta[:, 7] = [1 if f else 0 for f in flips]
    bounds, k = _resample_coeffs(bx[:, [3, 2]].reshape(-1), S, ktaps)          # per image: w (axis 0), then h (axis 1)
    coef[..., :2], coef[..., 2:] = bounds.reshape(B, 2, S, 2), k.reshape(B, 2, S, ktaps)
    return host, int(bx[:, 2].max()), ktaps


def sample_resized_crops(sizes, scale=(0.2, 1.0), ratio=(3 / 4, 4 / 3), rng=np.random):
    """One (top, left, h, w) per (H, W) in sizes by torchvision's RandomResizedCrop.get_params: ten tries of target_area = H * W * U(scale) and
    aspect = exp(U(log ratio)), w = round(sqrt(area * aspect)), h = round(sqrt(area / aspect)), accepted when 0 < w <= W and 0 < h <= H with
    top uniform in [0, H - h] and left in [0, W - w]; otherwise the central crop with the image's ratio clamped into `ratio`.  Equal in
    DISTRIBUTION, not in random stream: torchvision draws from torch's generator, this from a numpy one."""
    out = []
    log_r = (np.log(ratio[0]), np.log(ratio[1]))
    for H, W in sizes:
        H, W = int(H), int(W)
        box = None
        for _ in range(10):
            area = H * W * float(rng.uniform(scale[0], scale[1]))
            aspect = float(np.exp(rng.uniform(log_r[0], log_r[1])))
            w, h = int(round(np.sqrt(area * aspect))), int(round(np.sqrt(area / aspect)))
            if 0 < w <= W and 0 < h <= H:
                box = (_randint(rng, H - h + 1), _randint(rng, W - w + 1), h, w)
                break
        if box is None:
            in_ratio = W / H
            if in_ratio < min(ratio):
                w, h = W, int(round(W / min(ratio)))
            elif in_ratio > max(ratio):
                h, w = H, int(round(H * max(ratio)))
            else:
                w, h = W, H
            box = ((H - h) // 2, (W - w) // 2, h, w)
        out.append(box)
    return out


def pack_images(images, device="cuda"):
    """A list of (H, W, 3) uint8 images -> (1-D uint8 device buffer holding them back to back, [(H, W), ...]).  numpy arrays / CPU tensors (what
    a decoder or np.asarray(PIL image) gives) are joined on the host and go up in ONE copy; a list of device tensors is joined on the device."""
    if len(images) == 0:
        raise ValueError("pack_images: no images")
    on_dev = [isinstance(im, torch.Tensor) and im.is_cuda for im in images]
    if any(on_dev) and not all(on_dev):
        raise ValueError("pack_images: host and device images in one list")
    sizes = []
    for i, im in enumerate(images):
        if im.ndim != 3 or im.shape[2] != 3:
            raise ValueError("pack_images: image %d must be (H, W, 3), got shape %s" % (i, tuple(im.shape)))
        if im.dtype not in (np.uint8, torch.uint8):
            raise ValueError("pack_images: image %d must hold uint8 pixels, got %s" % (i, im.dtype))
        sizes.append((int(im.shape[0]), int(im.shape[1])))
    if all(on_dev):
        return torch.cat([im.reshape(-1) for im in images]), sizes
    flat = np.concatenate([(im.numpy() if isinstance(im, torch.Tensor) else np.asarray(im)).reshape(-1) for im in images])
    return torch.from_numpy(flat).to(device), sizes


_image_ws = {}   # device -> the horizontal pass's intermediate rows, reused between calls (stream-ordered)


def prepare_pretrain_images(images, mean, std, crop_size=256, num_frm=4, scale=(0.2, 1.0), ratio=(3 / 4, 4 / 3), augment=None, rng=np.random,
                            crop_boxes=None, flips=None, aug_ops=None, boxes=None, assume_255=None, patch_size=16, device="cuda", **box_kw):
    """The image-text branch of a pretraining batch on the device (PretrainImageTextDataset, dataset_pretrain_sparse.py:125-193, then the
    collator and ImageNorm as for clips): images -- a list of decoded (H, W, 3) uint8 images of any sizes, or what pack_images returned -- go
    through RandomResizedCrop(crop_size, scale, ratio, BICUBIC) and RandomHorizontalFlip (alpro_resized_crop: PIL's arithmetic bit for bit),
    augment (a RandomAugment; None: no ops) at T = 1, are repeated to num_frm equal frames, and take prepare_pretrain_clips' path (random
    erase with `boxes` / box_kw, ImageNorm; uint8 always counts as 0..255).  -> prepare_pretrain_clips' dict plus crop_boxes, flips and
    aug_ops, with which (and `boxes`) a call can be replayed.  crop_boxes (top, left, h, w), flips and aug_ops are drawn from rng unless given."""
    from alpro_amd import hip
    packed, sizes = images if isinstance(images, tuple) else pack_images(images, device=device)
    B, S = len(sizes), int(crop_size)
    if crop_boxes is None:
        crop_boxes = sample_resized_crops(sizes, scale=scale, ratio=ratio, rng=rng)
    if flips is None:
        flips = [bool(rng.random() < 0.5) for _ in range(B)]
    if augment is not None and aug_ops is None:
        aug_ops = augment.sample(B, rng=rng)
    if augment is None and aug_ops is not None:
        raise ValueError("prepare_pretrain_images: aug_ops need augment= (a RandomAugment)")
    tmp = None
    if isinstance(packed, torch.Tensor) and packed.is_cuda and B and len(crop_boxes) == B:   # (anything else: resized_crop refuses it by name)
        need = B * max(int(bx[2]) for bx in crop_boxes) * 3 * max(S, 0)
        key = (packed.device.type, packed.device.index)
        tmp = _image_ws.get(key)
        if tmp is None or tmp.numel() < need:
            tmp = _image_ws[key] = torch.empty(need, dtype=torch.uint8, device=packed.device)
    img = hip.resized_crop(packed, sizes, crop_boxes, flips, S, tmp=tmp)
    if augment is not None:
        img = augment(img, ops=aug_ops)
    clips = img.repeat(1, int(num_frm), 1, 1, 1)
    out = prepare_pretrain_clips(clips, mean, std, patch_size=patch_size, boxes=boxes, rng=rng, assume_255=assume_255, **box_kw)
    out.update(crop_boxes=crop_boxes, flips=flips, aug_ops=aug_ops)
    return out
