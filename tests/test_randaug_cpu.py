"""CPU (no GPU): the host side of the device clip augmentation -- TemporalConsistentRandomAugment's surface and sampling, the
square-crop sampler, the C ABI of alpro_augment_stage / alpro_augment_stats -- and self-checks of the numpy oracle
(tests/randaug_cases.py) that tests/test_hip_randaug.py holds the kernel to."""
import inspect
import os
import re

import numpy as np
import pytest

from alpro_amd.hip import AUG_OPS                       # the oracle's op codes are the library's: every test here needs the augmentation surface
from tests import randaug_cases as rc
from tests.conftest import ROOT


def _aug(**kw):
    from alpro_amd.input_gpu import TemporalConsistentRandomAugment
    return TemporalConsistentRandomAugment(**kw)


# ---- surface ----------------------------------------------------------------------------------------------------------------------------
def test_constructor_keeps_the_reference_signature():
    from alpro_amd.input_gpu import TemporalConsistentRandomAugment
    sig = inspect.signature(TemporalConsistentRandomAugment.__init__)
    assert list(sig.parameters) == ["self", "N", "M", "p", "tensor_in_tensor_out", "augs"]
    d = {k: v.default for k, v in sig.parameters.items() if k != "self"}
    assert d == {"N": 2, "M": 10, "p": 0.0, "tensor_in_tensor_out": True, "augs": []}
    a = _aug(N=2, M=5, p=0.0, tensor_in_tensor_out=False, augs=["Identity", "Rotate"])
    assert (a.N, a.M, a.p, a.augs) == (2, 5, 0.0, ["Identity", "Rotate"])


def test_equalize_is_refused_and_empty_augs_is_the_thirteen_ops():
    with pytest.raises(ValueError, match="Equalize"):
        _aug(augs=["Identity", "Equalize"])
    with pytest.raises(ValueError, match="AutoContrast"):
        _aug(augs=["AutoContrast"])
    a = _aug()
    assert len(a.augs) == 13 and set(a.augs) == set(rc.OPS) and "Equalize" not in a.augs


def test_op_codes_match_the_header_and_the_oracle():
    from alpro_amd import hip
    assert hip.AUG_OPS == rc.OPS == AUG_OPS
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"ALPRO_AUG_([A-Z_]+) = (\d+)", hdr))
    names = {"IDENTITY": "Identity", "HFLIP": "HorizontalFlip", "BRIGHTNESS": "Brightness", "CONTRAST": "Contrast", "SHARPNESS": "Sharpness",
             "COLOR": "Color", "SOLARIZE": "Solarize", "POSTERIZE": "Posterize", "TRANSLATE_X": "TranslateX", "TRANSLATE_Y": "TranslateY",
             "SHEAR_X": "ShearX", "SHEAR_Y": "ShearY", "ROTATE": "Rotate"}
    assert {names[k]: v for k, v in enum.items()} == hip.AUG_OPS


def test_level_to_arguments():
    from alpro_amd.input_gpu import aug_op_args
    A = rc.OPS
    assert aug_op_args(A["Brightness"], 5) == (1.0, 0.0) and aug_op_args(A["Contrast"], 3)[0] == 3 / 10 * 1.8 + 0.1
    assert aug_op_args(A["Solarize"], 5)[0] == 128 and aug_op_args(A["Solarize"], 10)[0] == 256
    assert [aug_op_args(A["Posterize"], m)[0] for m in (3, 5, 8)] == [1, 2, 3]
    assert aug_op_args(A["TranslateX"], 3)[0] == 3.0 and aug_op_args(A["TranslateY"], 8)[0] == 8.0
    assert aug_op_args(A["ShearX"], 10)[0] == 0.3
    c, s = aug_op_args(A["Rotate"], 10)
    assert abs(c - np.sqrt(3) / 2) < 1e-15 and abs(s - 0.5) < 1e-15
    assert aug_op_args(A["Identity"], 7) == (0.0, 0.0) and aug_op_args(-1, 7) == (0.0, 0.0)


# ---- sampling ---------------------------------------------------------------------------------------------------------------------------
TEN = ["Identity", "Contrast", "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "HorizontalFlip"]


def test_sample_draws_n_distinct_ops_per_clip():
    a = _aug(N=3, M=5, augs=TEN)
    ops = a.sample(500, rng=np.random.RandomState(0))
    assert ops.shape == (500, 3) and ops.dtype == np.int32
    allowed = {rc.OPS[n] for n in TEN}
    for row in ops:
        assert len(set(row)) == 3 and set(row) <= allowed
    # numpy's Generator is taken as well as the legacy RandomState / module interface
    assert _aug(N=2, augs=TEN).sample(4, rng=np.random.default_rng(0)).shape == (4, 2)


def test_sample_with_p_one_skips_every_op():
    ops = _aug(N=2, M=5, p=1.0, augs=TEN).sample(64, rng=np.random.RandomState(1))
    assert ops.shape == (64, 2) and (ops == -1).all()


def test_sample_is_uniform_over_the_ops():
    N, B = 2, 20000
    ops = _aug(N=N, M=5, augs=TEN).sample(B, rng=np.random.RandomState(2))
    for name in TEN:
        share = float((ops == rc.OPS[name]).any(axis=1).mean())
        assert abs(share - N / 10) <= 0.05 * N / 10, (name, share)
    # with p = 0.5 about half of the drawn ops are skipped
    half = _aug(N=N, M=5, p=0.5, augs=TEN).sample(B, rng=np.random.RandomState(3))
    assert abs(float((half == -1).mean()) - 0.5) < 0.02


def test_square_crop_sampler_stays_in_range_and_reaches_both_ends():
    from alpro_amd.input_gpu import sample_square_crops
    crops = sample_square_crops(4000, 48, 70, 32, rng=np.random.RandomState(4))
    tops, lefts = np.array(crops).T
    assert len(crops) == 4000 and tops.min() == 0 and tops.max() == 16 and lefts.min() == 0 and lefts.max() == 38
    assert sample_square_crops(3, 32, 32, 32, rng=np.random.RandomState(5)) == [(0, 0)] * 3
    g = np.array(sample_square_crops(2000, 40, 36, 32, rng=np.random.default_rng(6)))
    assert g[:, 0].min() == 0 and g[:, 0].max() == 8 and g[:, 1].min() == 0 and g[:, 1].max() == 4
    with pytest.raises(ValueError, match="33"):
        sample_square_crops(1, 32, 64, 33)


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------
def test_augment_symbols_are_declared_and_exported_at_abi_22():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    for sym in ("alpro_augment_stage", "alpro_augment_stats"):
        assert re.search(r"\bint %s\s*\(" % sym, hdr), sym
        assert sym in hip.EXPORTS
        assert hasattr(hip.load(), sym)
    assert hip.ABI_VERSION == 22 and int(re.search(r"#define ALPRO_HIP_ABI_VERSION (\d+)", hdr).group(1)) == 22
    assert hip.load().alpro_hip_abi_version() == 22


def test_host_side_refusals_need_no_device():
    """What the library refuses before any launch: NULL pointers and a crop that does not fit, each naming the value."""
    import ctypes
    from alpro_amd import hip
    lib = hip.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.alpro_augment_stage(p, p, None, p, p, p, 1, 1, 8, 8, 9, 8, None) != 0
    assert "crop height 9" in lib.alpro_hip_last_error().decode()
    assert lib.alpro_augment_stage(p, p, None, p, p, p, 1, 1, 8, 8, 8, 4, None) != 0
    assert "no crop offsets" in lib.alpro_hip_last_error().decode()
    assert lib.alpro_augment_stage(p, p, None, p, p, p, 1, 1, 8, 8, 8, 8, None) != 0
    assert "overlaps" in lib.alpro_hip_last_error().decode()
    assert lib.alpro_augment_stats(p, None, p, p, None, p, 1, 1, 8, 8, 8, 8, None) != 0
    assert "NULL" in lib.alpro_hip_last_error().decode()
    import torch
    with pytest.raises(RuntimeError, match="cpu"):
        _aug(N=1, augs=["Identity"])(torch.zeros(1, 1, 3, 8, 8, dtype=torch.uint8))


# ---- oracle self-checks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", rc.SHAPES)
def test_oracle_integer_translate_is_a_shifted_copy_with_fill(H, W):
    img = rc.images(H, W)["noise"]
    for M in rc.LEVELS:
        o = M                                        # M / 10 * 10 for the integer levels used here
        ex = np.full_like(img, rc.FILL)
        ex[:, :, :W - o] = img[:, :, o:]
        assert np.array_equal(rc.apply_op(img, "TranslateX", M), ex)
        ey = np.full_like(img, rc.FILL)
        if o < H:
            ey[:, :H - o, :] = img[:, o:, :]
        assert np.array_equal(rc.apply_op(img, "TranslateY", M), ey)


@pytest.mark.parametrize("H,W", rc.SHAPES)
def test_oracle_identities(H, W):
    for kind, img in rc.images(H, W).items():
        assert np.array_equal(rc.apply_op(rc.apply_op(img, "HorizontalFlip", 5), "HorizontalFlip", 5), img)
        assert np.array_equal(rc.apply_op(img, "Brightness", 5), img)       # f == 1 at M = 5
        assert np.array_equal(rc.apply_op(img, "Sharpness", 5), img)
        assert np.array_equal(rc.apply_op(img, "Identity", 8), img)
    flat = np.full((3, H, W), rc.FILL, dtype=np.uint8)
    for M in rc.LEVELS:
        for name in ("Rotate", "ShearX", "ShearY"):
            assert np.array_equal(rc.apply_op(flat, name, M), flat)          # the fill equals the image: nothing can change


def test_oracle_pointwise_ops_on_hand_values():
    img = np.zeros((3, 4, 4), dtype=np.uint8)
    img[0], img[1], img[2] = 10, 100, 250
    assert rc.apply_op(img, "Solarize", 5)[:, 0, 0].tolist() == [10, 100, 5]            # t = 128
    assert rc.apply_op(img, "Posterize", 5)[:, 0, 0].tolist() == [0, 64, 192]           # 2 bits kept
    assert rc.apply_op(img, "Brightness", 8)[:, 0, 0].tolist() == [15, 154, 255]        # f = 1.54, truncated, saturated
    # constant channels: mean = 10 * .114 + 100 * .587 + 250 * .299 = 134.59; (el - mean) * 0.64 + mean
    assert rc.apply_op(img, "Contrast", 3)[:, 0, 0].tolist() == [54, 112, 208]
    # a flat image has deg == src: the blend returns src for every f
    assert np.array_equal(rc.apply_op(img, "Sharpness", 8), img)
    # grey pixels keep their value under Color up to the truncation of 3 products (weights sum to 1)
    grey = np.full((3, 2, 2), 77, dtype=np.uint8)
    assert np.abs(rc.apply_op(grey, "Color", 8).astype(int) - 77).max() <= 1
    # rotation by 30 degrees (M = 10) about (W/2, H/2): the centre pixel's source is itself
    H = W = 9
    dot = np.zeros((3, H, W), dtype=np.uint8)
    rot = rc.apply_op(dot, "Rotate", 10)
    assert rot[0, 4, 4] == 0 and rot[0, 0, 0] == rc.FILL                                  # the corner looks outside: fill
