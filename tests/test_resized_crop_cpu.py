"""CPU (no GPU): the host side of the image-text stream's device preparation -- PIL's 8-bit bicubic coefficients
(alpro_amd.input_gpu.resample_coeffs) and the numpy restatement of the two integer passes (tests/resized_crop_cases.py) against
PIL itself, bit for bit; the RandomResizedCrop box sampler; RandomAugment's sampling; the table alpro_resized_crop reads; its C ABI
and the wrappers' refusals that need no device."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from alpro_amd.input_gpu import RandomAugment, resample_coeffs, resample_ksize, resample_table, sample_resized_crops   # every test here needs the surface
from tests import resized_crop_cases as cc
from tests.conftest import ROOT

EIGHT = ["Identity", "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"]   # dataset_pretrain_sparse.py:137


# ---- coefficients + restatement == PIL --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", cc.SIZES)
def test_restatement_equals_pil_bit_for_bit(H, W):
    for kind in ("noise", "ramp"):
        img = cc.image(H, W, kind)
        pil = Image.fromarray(img)
        for S in cc.OUT_SIZES:
            for (top, left, h, w) in cc.boxes(H, W):
                ref = np.asarray(pil.crop((left, top, left + w, top + h)).resize((S, S), Image.BICUBIC))
                got = cc.resized_crop(img, (top, left, h, w), S)
                d = np.abs(ref.astype(np.int32) - got.astype(np.int32))
                assert d.max() == 0, (kind, S, (top, left, h, w), int(d.max()), float((d > 0).mean()))


def test_flip_mirrors_the_columns_as_pil_does():
    img = cc.image(37, 53, "noise")
    box = cc.boxes(37, 53)[4]
    top, left, h, w = box
    ref = np.asarray(Image.fromarray(img).crop((left, top, left + w, top + h)).resize((32, 32), Image.BICUBIC).transpose(Image.FLIP_LEFT_RIGHT))
    assert np.array_equal(cc.resized_crop(img, box, 32, flip=True), ref)


def test_coefficient_properties():
    """Taps stay inside the extent, the identity at in == out, the tap slots the formula names, the int32 bound for the largest table."""
    for n_in, n_out in [(1, 8), (7, 8), (32, 32), (53, 8), (500, 32), (640, 256), (4096, 64)]:
        bounds, k = resample_coeffs(n_in, n_out)
        assert bounds.dtype == np.int32 and k.dtype == np.int32 and bounds.shape == (n_out, 2) and k.shape == (n_out, resample_ksize(n_in, n_out))
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(axis=1) <= n_in).all()
        for xx, (first, n) in enumerate(bounds):
            assert not k[xx, n:].any()
            assert abs(int(k[xx].astype(np.int64).sum()) - (1 << 22)) <= k.shape[1]            # normalised weights, each rounded once
        assert int(np.abs(k.astype(np.int64)).sum(axis=1).max()) * 255 + (1 << 21) < 2 ** 31
    bounds, k = resample_coeffs(32, 32)
    for xx, (first, n) in enumerate(bounds):
        assert k[xx, xx - first] == 1 << 22 and np.count_nonzero(k[xx]) == 1
    assert resample_ksize(500, 32) == 65 and resample_ksize(20, 32) == 5 and resample_ksize(4096, 64) == 257


def test_table_layout():
    """[meta int64 (B, 8) | coef int32 (B, 2, S, 2 + ktaps)], offsets running over the packed images, short rows zero-padded."""
    sizes, boxes, S = [(37, 53), (300, 500)], [(1, 2, 20, 30), (0, 0, 300, 500)], 32
    host, max_h, ktaps = resample_table(sizes, boxes, [True, False], S)
    assert host.dtype == np.uint8 and (max_h, ktaps) == (300, 65) and host.size == 2 * 64 + 2 * 2 * S * 67 * 4
    meta = host[:128].view(np.int64).reshape(2, 8)
    assert meta.tolist() == [[0, 37, 53, 1, 2, 20, 30, 1], [37 * 53 * 3, 300, 500, 0, 0, 300, 500, 0]]
    coef = host[128:].view(np.int32).reshape(2, 2, S, 67)
    for b, axis, extent in [(0, 0, 30), (0, 1, 20), (1, 0, 500), (1, 1, 300)]:
        bounds, k = resample_coeffs(extent, S)
        assert np.array_equal(coef[b, axis, :, :2], bounds) and np.array_equal(coef[b, axis, :, 2:2 + k.shape[1]], k)
        assert not coef[b, axis, :, 2 + k.shape[1]:].any()


# ---- RandomResizedCrop.get_params ------------------------------------------------------------------------------------------------------
def test_crop_sampler_boxes_lie_inside_their_images():
    sizes = cc.SIZES * 20
    for (H, W), (top, left, h, w) in zip(sizes, sample_resized_crops(sizes, rng=np.random.RandomState(0))):
        assert 1 <= h <= H and 1 <= w <= W and 0 <= top <= H - h and 0 <= left <= W - w, ((H, W), (top, left, h, w))
    assert len(sample_resized_crops(cc.SIZES, rng=np.random.default_rng(0))) == len(cc.SIZES)     # numpy's Generator is taken as well


def test_crop_sampler_fallback_is_the_central_crop_with_the_ratio_clamped():
    # H = 10, W = 1000: every try has h >= sqrt(0.2 * 10000 / (4/3)) = 38.7 > 10; in_ratio 100 > 4/3 -> h = 10, w = round(10 * 4/3) = 13, centred
    # H = 1000, W = 10: in_ratio 0.01 < 3/4 -> w = 10, h = round(10 / (3/4)) = 13, centred
    for seed in range(5):
        assert sample_resized_crops([(10, 1000), (1000, 10)], rng=np.random.RandomState(seed)) == [(0, 493, 10, 13), (493, 0, 13, 10)]


def test_crop_sampler_area_and_ratio_ranges():
    H, W = 300, 400
    bx = np.array(sample_resized_crops([(H, W)] * 2000, rng=np.random.RandomState(1)), dtype=np.float64)
    top, left, h, w = bx.T
    # w = round(sqrt(area * aspect)) and h = round(sqrt(area / aspect)) each move by at most 0.5: area by at most (w + h) / 2 + 0.25,
    # and the ratio w / h stays within (w -+ 0.5) / (h +- 0.5) of a value in [3/4, 4/3]
    slack = (w + h) / 2 + 0.25
    assert (w * h >= 0.2 * H * W - slack).all() and (w * h <= 1.0 * H * W + slack).all()
    assert ((w + 0.5) / (h - 0.5) >= 3 / 4).all() and ((w - 0.5) / (h + 0.5) <= 4 / 3).all()
    assert (w * h).min() < 0.3 * H * W and (w * h).max() > 0.9 * H * W                      # the range is used, not a corner of it
    assert (w / h).min() < 0.85 and (w / h).max() > 1.2
    assert top.min() == 0 and left.min() == 0 and (top + h).max() == H and (left + w).max() == W


def test_crop_sampler_is_reproducible():
    a = sample_resized_crops(cc.SIZES * 3, rng=np.random.RandomState(5))
    assert a == sample_resized_crops(cc.SIZES * 3, rng=np.random.RandomState(5))
    assert a != sample_resized_crops(cc.SIZES * 3, rng=np.random.RandomState(6))


# ---- RandomAugment ------------------------------------------------------------------------------------------------------------------------
def test_random_augment_keeps_the_reference_signature():
    sig = inspect.signature(RandomAugment.__init__)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == {"N": 2, "M": 10, "isPIL": False, "augs": []}
    a = RandomAugment(2, 7, isPIL=True, augs=EIGHT)
    assert (a.N, a.M, a.augs) == (2, 7, EIGHT)
    assert len(RandomAugment().augs) == 13


def test_random_augment_samples_with_replacement_and_applies_half():
    from alpro_amd.hip import AUG_OPS
    a = RandomAugment(2, 7, isPIL=True, augs=EIGHT)
    ops = a.sample(2000, rng=np.random.RandomState(0))
    assert ops.shape == (2000, 2) and ops.dtype == np.int32
    assert set(ops.ravel()) <= {-1} | {AUG_OPS[n] for n in EIGHT}
    skipped = float((ops == -1).mean())
    assert 0.44 <= skipped <= 0.56, skipped
    # both entries equal: only possible with replacement; counted over the rows where neither was skipped (rate 1/8)
    full = a.sample(2000, rng=np.random.RandomState(1))
    kept = full[(full >= 0).all(axis=1)]
    same = float((kept[:, 0] == kept[:, 1]).mean())
    assert len(kept) > 300 and 0.08 <= same <= 0.18, (len(kept), same)
    # the draw itself, before the skips: PROB = 1 applies every op
    always = RandomAugment(2, 7, augs=EIGHT)
    always.PROB = 1.0
    drawn = always.sample(2000, rng=np.random.RandomState(2))
    assert (drawn >= 0).all() and 0.08 <= float((drawn[:, 0] == drawn[:, 1]).mean()) <= 0.18
    assert RandomAugment(3, 7, augs=["Rotate"]).sample(4, rng=np.random.default_rng(0)).shape == (4, 3)    # N may exceed the op count


def test_random_augment_refuses_equalize_and_unknown_names():
    with pytest.raises(ValueError, match="'Equalize' is not built on the device"):
        RandomAugment(augs=["Identity", "Equalize"])
    with pytest.raises(ValueError, match="unknown op 'AutoContrast'"):
        RandomAugment(augs=["AutoContrast"])


# ---- ABI and refusals without a device ----------------------------------------------------------------------------------------------------
def test_resized_crop_is_declared_and_exported_at_abi_22():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    assert re.search(r"\bint alpro_resized_crop\s*\(", hdr) and "alpro_resized_crop" in hip.EXPORTS and hasattr(hip.load(), "alpro_resized_crop")
    assert hip.ABI_VERSION == 22 and int(re.search(r"#define ALPRO_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 22
    assert hip.load().alpro_hip_abi_version() == 22
    assert int(re.search(r"#define ALPRO_RESAMPLE_MAX_TAPS (\d+)", hdr).group(1)) == hip.RESAMPLE_MAX_TAPS >= resample_ksize(4096, 64)


def test_library_refuses_before_any_launch():
    import ctypes
    from alpro_amd import hip
    lib = hip.load()
    buf = ctypes.create_string_buffer(1 << 16)
    base = ctypes.addressof(buf)
    p = lambda o: ctypes.c_void_p(base + o)   # noqa: E731
    src, meta, coef, tmp, dst = p(0), p(4096), p(8192), p(16384), p(32768)
    assert lib.alpro_resized_crop(src, 3000, meta, coef, tmp, dst, 1, 30, 8, 5, None) != 0
    assert "output size 30" in lib.alpro_hip_last_error().decode()
    assert lib.alpro_resized_crop(src, 3000, meta, coef, tmp, dst, 1, 8, 8, hip.RESAMPLE_MAX_TAPS + 1, None) != 0
    assert "ktaps %d" % (hip.RESAMPLE_MAX_TAPS + 1) in lib.alpro_hip_last_error().decode()
    assert lib.alpro_resized_crop(src, 3000, meta, coef, tmp, p(1000), 1, 8, 8, 5, None) != 0
    assert "dst overlaps src" in lib.alpro_hip_last_error().decode()
    assert lib.alpro_resized_crop(src, 3000, meta, coef, p(32768 + 64), dst, 1, 8, 8, 5, None) != 0
    assert "tmp overlaps" in lib.alpro_hip_last_error().decode()
    assert lib.alpro_resized_crop(src, 3000, meta, coef, p(16385), dst, 1, 8, 8, 5, None) != 0
    assert "aligned" in lib.alpro_hip_last_error().decode()
    assert lib.alpro_resized_crop(src, 3000, None, coef, tmp, dst, 1, 8, 8, 5, None) != 0
    assert "NULL" in lib.alpro_hip_last_error().decode()


def test_wrappers_refuse_cpu_tensors():
    from alpro_amd import hip
    from alpro_amd.input_gpu import pack_images, prepare_pretrain_images
    flat = torch.zeros(8 * 8 * 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match=r"got cpu \(no CPU fallback\)"):
        hip.resized_crop(flat, [(8, 8)], [(0, 0, 8, 8)], [False], 8)
    packed, sizes = pack_images([np.zeros((8, 8, 3), np.uint8), torch.zeros(4, 6, 3, dtype=torch.uint8)], device="cpu")
    assert sizes == [(8, 8), (4, 6)] and packed.shape == (8 * 8 * 3 + 4 * 6 * 3,)
    with pytest.raises(RuntimeError, match=r"got cpu \(no CPU fallback\)"):
        prepare_pretrain_images((packed, sizes), [0.5] * 3, [0.5] * 3, crop_size=8, num_frm=2, rng=np.random.RandomState(0))
    with pytest.raises(RuntimeError, match=r"RandomAugment needs a device tensor, got cpu \(no CPU fallback\)"):
        RandomAugment(1, 7, augs=["Rotate"])(torch.zeros(1, 1, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="float32"):
        pack_images([np.zeros((8, 8, 3), np.float32)])
    with pytest.raises(ValueError, match=r"\(8, 8\)"):
        pack_images([np.zeros((8, 8), np.uint8)])
