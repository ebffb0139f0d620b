"""GPU: alpro_augment_stage / alpro_augment_stats (csrc/augment.hip) and their Python surface in alpro_amd/input_gpu.py against the
numpy restatement of tests/randaug_cases.py.

Shapes: B = 3 clips of T = 2 frames at 37 x 53 (odd and non-square: byte items at both ends of every row, rows that start on any
byte of a word, waves that straddle rows and planes), 64 x 64 (every item a whole word) and 16 x 200 (rows longer than a wave's
span of 256 pixels); a seeded-noise and a smooth ramp image each; levels 3, 5 and 8.

Bounds.  The integer ops, the table ops, Brightness and Sharpness (fp32 with one rounding per operation on both sides) and the
translations by whole pixels must match the oracle exactly.  ShearX, ShearY, Rotate and Color are evaluated in fp32 on the device
and in fp64 by the oracle: a value whose exact result lies within fp32 rounding of a half-way point (bilinear) or of an integer
(Color truncates) may land on the other side, by one grey level and never more; half-way blends are frequent for shear, whose
fractional source offsets at these levels are multiples of 0.01, so the share of such elements is capped at 5 % (a CPU comparison
of an fp32 against an fp64 restatement on these inputs stayed at 2.8 % or less for shear, 0.06 % or less for rotation).  A wrong
tap, sign, centre or fill moves noise-image pixels by tens of levels."""
import functools

import numpy as np
import pytest
import torch

from alpro_amd.input_gpu import aug_op_args
from tests import randaug_cases as rc

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


@functools.lru_cache(maxsize=None)
def _clips(H, W, kind):
    """(B, T, 3, H, W) uint8 numpy, read-only: the shape's image, rolled differently for every clip and frame so that no two are equal."""
    img = rc.images(H, W)[kind]
    out = np.stack([np.stack([np.roll(img, (3 * b + t, 5 * b + 2 * t), axis=(1, 2)) for t in range(rc.T)]) for b in range(rc.B)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expected(H, W, kind, name, M):
    ref = np.stack([rc.apply_clip(c, name, M) for c in _clips(H, W, kind)])
    ref.setflags(write=False)
    return ref


def _stage(x, codes, M, crop=None, out_hw=None):
    """One op stage through the raw entry points: codes (B) per clip, -1 = copy."""
    from alpro_amd import hip
    B, T = x.shape[:2]
    ops = torch.tensor(list(codes), dtype=torch.int32, device="cuda")
    args = torch.tensor([aug_op_args(int(c), M) for c in codes], dtype=torch.float64, device="cuda")
    crop_d = None if crop is None else torch.tensor(crop, dtype=torch.int32, device="cuda")
    sums, tables = hip.augment_buffers(B, T, x.device)
    hip.augment_stats(x, ops, args, sums, tables, crop=crop_d, out_hw=out_hw)
    return hip.augment_stage(x, ops, args, tables, crop=crop_d, out_hw=out_hw)


def _report(tag, got, ref):
    d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    print("%-40s max |diff| %3d   differing %.4f %%" % (tag, d.max(), 100.0 * (d > 0).mean()))
    return d


# ---- 1. every op alone against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", rc.SHAPES)
@pytest.mark.parametrize("name", rc.EXACT_OPS)
def test_exact_ops_match_the_oracle(name, H, W):
    for kind in ("noise", "ramp"):
        x = torch.from_numpy(_clips(H, W, kind).copy()).cuda()
        for M in rc.LEVELS:
            got = _stage(x, [rc.OPS[name]] * rc.B, M).cpu().numpy()
            d = _report("%s M=%d %dx%d %s" % (name, M, H, W, kind), got, _expected(H, W, kind, name, M))
            assert d.max() == 0


@pytest.mark.parametrize("H,W", rc.SHAPES)
@pytest.mark.parametrize("name", rc.CLOSE_OPS)
def test_bilinear_ops_and_color_within_one_level(name, H, W):
    for kind in ("noise", "ramp"):
        x = torch.from_numpy(_clips(H, W, kind).copy()).cuda()
        for M in rc.LEVELS:
            got = _stage(x, [rc.OPS[name]] * rc.B, M).cpu().numpy()
            d = _report("%s M=%d %dx%d %s" % (name, M, H, W, kind), got, _expected(H, W, kind, name, M))
            assert d.max() <= 1
            assert (d > 0).mean() <= 0.05


def test_contrast_sums_are_exact():
    """The statistics launch: integer channel sums of every Contrast frame, other clips' rows untouched."""
    from alpro_amd import hip
    H, W = 37, 53
    clips = _clips(H, W, "noise")
    x = torch.from_numpy(clips.copy()).cuda()
    codes = [rc.OPS["Contrast"], rc.OPS["Rotate"], rc.OPS["Contrast"]]
    ops = torch.tensor(codes, dtype=torch.int32, device="cuda")
    args = torch.tensor([aug_op_args(c, 3) for c in codes], dtype=torch.float64, device="cuda")
    sums, tables = hip.augment_buffers(rc.B, rc.T, x.device)
    sums.fill_(-7)
    hip.augment_stats(x, ops, args, sums, tables)
    got = sums.view(rc.B, rc.T, 3).cpu().numpy()
    ref = clips.astype(np.int64).sum(axis=(-1, -2))
    assert np.array_equal(got[[0, 2]], ref[[0, 2]]) and (got[1] == -7).all()


# ---- 2. temporal consistency and batching -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", rc.SHAPES)
def test_mixed_batch_equals_single_clip_launches_and_frames_agree(H, W):
    x = torch.from_numpy(_clips(H, W, "noise").copy()).cuda()
    for codes in ([rc.OPS["Rotate"], rc.OPS["Contrast"], rc.OPS["Sharpness"]], [rc.OPS["ShearY"], -1, rc.OPS["HorizontalFlip"]]):
        mixed = _stage(x, codes, 8)
        for b, c in enumerate(codes):
            single = _stage(x[b:b + 1].contiguous(), [c], 8)
            assert torch.equal(mixed[b:b + 1], single), (codes, b)
            for t in range(rc.T):     # each frame alone gives the frame of the clip: nothing leaks between the frames of a clip
                frame = _stage(x[b:b + 1, t:t + 1].contiguous(), [c], 8)
                assert torch.equal(mixed[b:b + 1, t:t + 1], frame), (codes, b, t)
    # the same frame twice in a clip comes out twice the same
    twin = x[:, :1].expand(-1, 2, -1, -1, -1).contiguous()
    out = _stage(twin, [rc.OPS["ShearX"], rc.OPS["Contrast"], rc.OPS["Color"]], 3)
    assert torch.equal(out[:, 0], out[:, 1])


# ---- 3. chain ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", rc.SHAPES)
def test_chain_equals_stage_after_stage(H, W):
    from alpro_amd.input_gpu import TemporalConsistentRandomAugment
    O = rc.OPS
    ops = [[O["ShearX"], O["Rotate"]], [O["Contrast"], -1], [O["HorizontalFlip"], O["TranslateY"]]]
    x = torch.from_numpy(_clips(H, W, "noise").copy()).cuda()
    keep = x.clone()
    aug = TemporalConsistentRandomAugment(N=2, M=8)
    got = aug(x, ops=ops)
    want = _stage(_stage(x, [o[0] for o in ops], 8), [o[1] for o in ops], 8)
    assert got.dtype == torch.uint8 and got.shape == x.shape and got.data_ptr() != x.data_ptr()
    assert torch.equal(got, want) and torch.equal(x, keep)
    assert torch.equal(aug(x, ops=ops), want)                        # a second call reuses the intermediate buffer
    # two resamplings with a uint8 image in between, not one composed warp: clip 0 against the oracle applied twice
    ref = np.stack([rc.apply_clip(rc.apply_clip(c, "ShearX", 8), "Rotate", 8) for c in _clips(H, W, "noise")[:1]])
    d = _report("ShearX>Rotate M=8 %dx%d" % (H, W), got[:1].cpu().numpy(), ref)
    assert d.max() <= 2       # stage 2 blends stage 1's differences (<= 1, convex weights) and may add one of its own; a composed warp is off by tens
    # every op skipped: a copy in a new tensor; sampled ops are reproducible from the generator
    none = aug(x, ops=[[-1, -1]] * rc.B)
    assert torch.equal(none, x) and none.data_ptr() != x.data_ptr()
    a = TemporalConsistentRandomAugment(N=2, M=5)
    assert torch.equal(a(x, rng=np.random.RandomState(7)), a(x, ops=a.sample(rc.B, rng=np.random.RandomState(7))))


# ---- 4. fused crop ------------------------------------------------------------------------------------------------------------------------
def test_fused_crop_equals_slicing_first():
    from alpro_amd.input_gpu import TemporalConsistentRandomAugment
    rng = np.random.RandomState(11)
    src = torch.from_numpy(rng.randint(0, 256, (rc.B, rc.T, 3, 48, 70)).astype(np.uint8)).cuda()
    offs = [(0, 0), (16, 38), (7, 13)]
    sliced = torch.stack([src[b, :, :, t:t + 32, l:l + 32] for b, (t, l) in enumerate(offs)]).contiguous()
    for name in ("Rotate", "Sharpness", "Contrast", "HorizontalFlip", "Identity"):
        for M in (3, 8):
            fused = _stage(src, [rc.OPS[name]] * rc.B, M, crop=offs, out_hw=(32, 32))
            assert fused.shape == (rc.B, rc.T, 3, 32, 32)
            assert torch.equal(fused, _stage(sliced, [rc.OPS[name]] * rc.B, M)), (name, M)
    # through the augmenter, with a crop whose rows are not whole words
    aug = TemporalConsistentRandomAugment(N=2, M=8)
    ops = [[rc.OPS["Rotate"], rc.OPS["Sharpness"]]] * rc.B
    offs30 = [(0, 0), (18, 40), (7, 13)]
    sl30 = torch.stack([src[b, :, :, t:t + 30, l:l + 30] for b, (t, l) in enumerate(offs30)]).contiguous()
    assert torch.equal(aug(src, ops=ops, crop_size=30, crop_offsets=offs30), aug(sl30, ops=ops))
    drawn = aug(src, ops=[[-1, -1]] * rc.B, crop_size=32, rng=np.random.RandomState(3))      # offsets from the generator, crop only
    from alpro_amd.input_gpu import sample_square_crops
    o = sample_square_crops(rc.B, 48, 70, 32, rng=np.random.RandomState(3))
    assert torch.equal(drawn, torch.stack([src[b, :, :, t:t + 32, l:l + 32] for b, (t, l) in enumerate(o)]))


# ---- 5. prepare_pretrain_clips ----------------------------------------------------------------------------------------------------------
def test_prepare_pretrain_clips_with_augmenter_and_unchanged_default():
    from alpro_amd import hip
    from alpro_amd.input_gpu import TemporalConsistentRandomAugment, prepare_pretrain_clips, sample_erase_box
    rng = np.random.RandomState(12)
    raw = torch.from_numpy(rng.randint(0, 256, (rc.B, rc.T, 3, 48, 70)).astype(np.uint8)).cuda()
    aug = TemporalConsistentRandomAugment(N=2, M=5, augs=["Identity", "Contrast", "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX",
                                                          "TranslateY", "Rotate", "HorizontalFlip"])
    boxes = [sample_erase_box(32, 32, 16, rng=np.random.RandomState(2)) for _ in range(rc.B)]
    out = prepare_pretrain_clips(raw, MEAN, STD, boxes=boxes, augment=aug, crop_size=32, rng=np.random.RandomState(5))
    assert out["aug_ops"].shape == (rc.B, 2) and len(out["crop_offsets"]) == rc.B
    mid = aug(raw, ops=out["aug_ops"], crop_size=32, crop_offsets=out["crop_offsets"])
    plain = prepare_pretrain_clips(mid, MEAN, STD, boxes=boxes)
    assert out["visual_inputs"].shape == (rc.B, rc.T, 3, 32, 32)
    for k in ("visual_inputs", "crop_visual_inputs", "context_visual_inputs", "mpm_mask"):
        assert torch.equal(out[k], plain[k]), k
    replay = prepare_pretrain_clips(raw, MEAN, STD, boxes=boxes, augment=aug, crop_size=32, aug_ops=out["aug_ops"], crop_offsets=out["crop_offsets"])
    assert torch.equal(replay["visual_inputs"], out["visual_inputs"])
    # defaults: what the function gave before it knew about augmentation -- alpro_prepare_clips on the raw input, and only its keys
    raw224 = torch.from_numpy(rng.randint(0, 256, (2, 2, 3, 64, 64)).astype(np.uint8)).cuda()
    bx = [sample_erase_box(64, 64, 16, rng=np.random.RandomState(3)) for _ in range(2)]
    dflt = prepare_pretrain_clips(raw224, MEAN, STD, boxes=bx, augment=None, crop_size=None)
    vis, crop, ctx = hip.prepare_clips(raw224, MEAN, STD, 1.0 / 255.0, boxes=torch.tensor(bx, dtype=torch.int32, device="cuda"))
    assert sorted(dflt) == ["boxes", "context_visual_inputs", "crop_visual_inputs", "mpm_mask", "visual_inputs"]
    assert torch.equal(dflt["visual_inputs"], vis) and torch.equal(dflt["crop_visual_inputs"], crop) and torch.equal(dflt["context_visual_inputs"], ctx)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_value():
    from alpro_amd.input_gpu import TemporalConsistentRandomAugment, prepare_pretrain_clips
    aug = TemporalConsistentRandomAugment(N=1, M=5, augs=["Rotate"])
    x = torch.zeros(2, 2, 3, 48, 70, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="cpu"):
        aug(x.cpu())
    with pytest.raises(RuntimeError, match="float32"):
        aug(x.float())
    with pytest.raises(RuntimeError, match="contiguous.*strides"):
        aug(x[..., ::2])
    with pytest.raises(ValueError, match="crop_size 49 does not fit the 48 x 70 frame"):
        aug(x, crop_size=49)
    with pytest.raises(ValueError, match=r"\(17, 0\) of clip 1"):
        aug(x, crop_size=32, crop_offsets=[(0, 0), (17, 0)])
    with pytest.raises(ValueError, match="crop_size 30 is not a multiple of 4"):
        prepare_pretrain_clips(x, MEAN, STD, augment=aug, crop_size=30)
    with pytest.raises(ValueError, match="need augment"):
        prepare_pretrain_clips(x, MEAN, STD, crop_size=32)
    # the raw entry points refuse the same inputs themselves
    from alpro_amd import hip
    ops = torch.zeros(2, dtype=torch.int32, device="cuda")
    args = torch.zeros(2, 2, dtype=torch.float64, device="cuda")
    sums, tables = hip.augment_buffers(2, 2, x.device)
    with pytest.raises(RuntimeError, match="cpu"):
        hip.augment_stage(x.cpu(), ops, args, tables)
    with pytest.raises(RuntimeError, match="float32"):
        hip.augment_stage(x.float(), ops, args, tables)
    with pytest.raises(RuntimeError, match="49 x 32 does not fit the 48 x 70 frame"):
        hip.augment_stage(x, ops, args, tables, crop=torch.zeros(2, 2, dtype=torch.int32, device="cuda"), out_hw=(49, 32))
    with pytest.raises(RuntimeError, match="overlaps"):
        hip.augment_stage(x, ops, args, tables, dst=x)
