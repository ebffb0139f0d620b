"""Helper (no tests): a numpy restatement of the integer two-pass resampling alpro_resized_crop runs on the device, fed
with the product's own coefficients (alpro_amd.input_gpu.resample_coeffs), plus the images, output sizes and boxes the tests share.

An image is (H, W, 3) uint8 interleaved, as np.asarray(PIL image) gives it.  tests/test_resized_crop_cpu.py holds coefficients plus
restatement to PIL's Image.crop().resize(BICUBIC) bit for bit; tests/test_hip_resized_crop.py holds the kernel to the restatement."""
import functools

import numpy as np

PRECISION_BITS = 22
SIZES = [(37, 53), (300, 500), (64, 48), (20, 20), (480, 640), (17, 256), (33, 9), (32, 32), (1, 7)]   # (H, W)
OUT_SIZES = [8, 32, 64, 256]
GPU_SIZES = [(37, 53), (64, 48), (20, 20), (300, 500), (33, 9)]     # one packed batch
GPU_OUT_SIZES = [8, 32, 64]


@functools.lru_cache(maxsize=None)
def image(H, W, kind):
    """'noise': seeded uniform noise; 'ramp': a smooth two-way ramp, different per channel (randaug_cases.images, interleaved).  Read-only."""
    rng = np.random.RandomState(1000 * H + W)
    if kind == "noise":
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    else:
        y, x = np.mgrid[0:H, 0:W]
        img = np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(H + W - 2, 1)], axis=-1).astype(np.uint8)
    img.setflags(write=False)
    return img


def boxes(H, W, seed=0):
    """(top, left, h, w): the full image, a 1 x 1 crop, a full-height 1-column crop, the bottom-right corner crop, four seeded random boxes."""
    rng = np.random.RandomState(seed + 7 * H + W)
    out = [(0, 0, H, W), (H // 2, W // 3, 1, 1), (0, W - 1, H, 1), (H - (H + 1) // 2, W - (W + 1) // 2, (H + 1) // 2, (W + 1) // 2)]
    for _ in range(4):
        h, w = rng.randint(1, H + 1), rng.randint(1, W + 1)
        out.append((rng.randint(0, H - h + 1), rng.randint(0, W - w + 1), h, w))
    return out


def _pass(pix, bounds, k):
    """One pass along axis 0 of pix (in, ...) uint8 -> (out, ...) uint8: clip8((2^21 + sum_x k[xx, x] * pix[first + x]) >> 22), int32 wrap-free."""
    out = np.zeros((bounds.shape[0],) + pix.shape[1:], dtype=np.uint8)
    for xx, (first, n) in enumerate(bounds):
        kk = k[xx, :n].astype(np.int64).reshape((n,) + (1,) * (pix.ndim - 1))
        acc = (pix[first:first + n].astype(np.int64) * kk).sum(axis=0) + (1 << (PRECISION_BITS - 1))
        assert np.abs(kk).sum() * 255 + (1 << (PRECISION_BITS - 1)) < 2 ** 31     # PIL's and the kernel's int32 accumulator holds every partial sum
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resized_crop(img, box, S, flip=False):
    """(H, W, 3) uint8, box (top, left, h, w) -> (S, S, 3) uint8: the horizontal pass over the crop's columns, the uint8 intermediate, then
    the vertical pass; both passes always run (with equal sizes the coefficients are the identity); the flip mirrors the columns."""
    from alpro_amd.input_gpu import resample_coeffs
    top, left, h, w = box
    crop = img[top:top + h, left:left + w]
    tmp = _pass(crop.transpose(1, 0, 2), *resample_coeffs(w, S)).transpose(1, 0, 2)      # (h, S, 3)
    out = _pass(tmp, *resample_coeffs(h, S))                                             # (S, S, 3)
    return out[:, ::-1].copy() if flip else out


def planar(out):
    """(S, S, 3) -> (1, 3, S, S), the layout of one image in alpro_resized_crop's dst."""
    return np.ascontiguousarray(out.transpose(2, 0, 1))[None]
