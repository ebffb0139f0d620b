"""GPU: alpro_resized_crop (csrc/resample.hip) and prepare_pretrain_images against the numpy restatement of tests/resized_crop_cases.py,
which tests/test_resized_crop_cpu.py holds to PIL's Image.crop().resize(BICUBIC) bit for bit.  Everything here is integer: every
comparison is exact.

One batch of five images of different sizes in one packed buffer -- 37 x 53, 64 x 48, 20 x 20, 300 x 500, 33 x 9 -- to S = 8, 32 and 64,
for each of eight box kinds (the full image, a 1 x 1 crop, a full-height 1-column crop, the bottom-right corner crop, four seeded random
boxes), flips on for images 0, 2 and 3.  That is the smallest set with: a non-zero offset for four images; taps cut at all four edges of
a crop (full image, corner crop) and crops whose neighbours in the image must NOT be read (1 x 1, 1-column); 65 tap slots (500 -> 32)
beside 5 (20 -> 32) in one launch, and 251 at 500 -> 8; up-scaling (20 -> 64, 9 -> 32); the identity axis (the 64 rows of the full 64 x 48
image at S = 64); a partial last workgroup (h * S and 3 * S * S / 4 are no multiples of 256 at h = 37, S = 8) and rows of the
workspace beyond an image's h (max_h = 300 beside h = 1)."""
import functools

import numpy as np
import pytest
import torch

from tests import resized_crop_cases as cc

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
FLIPS = [True, False, True, True, False]
KINDS = ["noise", "ramp", "noise", "ramp", "noise"]
NBOX = 8


def _images():
    return [cc.image(H, W, kind) for (H, W), kind in zip(cc.GPU_SIZES, KINDS)]


def _boxes(j):
    return [cc.boxes(H, W)[j] for H, W in cc.GPU_SIZES]


@functools.lru_cache(maxsize=None)
def _expected(S, j):
    """(5, 1, 3, S, S) uint8, read-only: the restatement of box kind j of every image, flipped as FLIPS says."""
    ref = np.stack([cc.planar(cc.resized_crop(img, box, S, flip=f)) for img, box, f in zip(_images(), _boxes(j), FLIPS)])
    ref.setflags(write=False)
    return ref


def _packed():
    from alpro_amd.input_gpu import pack_images
    return pack_images(_images())


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", cc.GPU_OUT_SIZES)
def test_mixed_batch_matches_the_restatement_bit_for_bit(S):
    from alpro_amd import hip
    packed, sizes = _packed()
    assert sizes == cc.GPU_SIZES and packed.numel() == sum(H * W * 3 for H, W in sizes)
    keep = packed.clone()
    for j in range(NBOX):
        got = hip.resized_crop(packed, sizes, _boxes(j), FLIPS, S)
        assert got.shape == (5, 1, 3, S, S) and got.dtype == torch.uint8
        d = np.abs(got.cpu().numpy().astype(np.int32) - _expected(S, j).astype(np.int32))
        print("S=%d box kind %d: max |diff| %d, differing %.4f %%" % (S, j, d.max(), 100.0 * (d > 0).mean()))
        assert d.max() == 0
    assert torch.equal(packed, keep)


@pytest.mark.parametrize("S", cc.GPU_OUT_SIZES)
def test_mixed_batch_equals_single_image_launches_and_reuses_its_workspace(S):
    from alpro_amd import hip
    from alpro_amd.input_gpu import pack_images
    packed, sizes = _packed()
    tmp = torch.empty(5 * 300 * 3 * S, dtype=torch.uint8, device="cuda")
    for j in (0, 3, 5):
        boxes = _boxes(j)
        mixed = hip.resized_crop(packed, sizes, boxes, FLIPS, S, tmp=tmp)
        for b, img in enumerate(_images()):
            one, size1 = pack_images([img])
            assert torch.equal(mixed[b:b + 1], hip.resized_crop(one, size1, boxes[b:b + 1], FLIPS[b:b + 1], S)), (j, b)
        # the workspace now holds this call's rows (and, beyond each image's h, an earlier call's): a second call gives the same bits
        assert torch.equal(hip.resized_crop(packed, sizes, boxes, FLIPS, S, tmp=tmp), mixed)
        assert torch.equal(hip.resized_crop(packed, sizes, boxes, None, S, tmp=tmp)[[1, 4]], mixed[[1, 4]])      # flips=None: none flipped


def test_device_images_pack_on_the_device():
    from alpro_amd import hip
    from alpro_amd.input_gpu import pack_images
    packed, sizes = _packed()
    on_dev, sizes_d = pack_images([torch.from_numpy(img.copy()).cuda() for img in _images()])
    assert sizes_d == sizes and torch.equal(on_dev, packed)
    assert torch.equal(hip.resized_crop(on_dev, sizes, _boxes(4), FLIPS, 32), torch.from_numpy(_expected(32, 4).copy()).cuda())


# ---- 2. prepare_pretrain_images -----------------------------------------------------------------------------------------------------------
def test_prepare_pretrain_images_equals_the_chain_by_hand():
    from alpro_amd import hip
    from alpro_amd.input_gpu import RandomAugment, TemporalConsistentRandomAugment, prepare_pretrain_clips, prepare_pretrain_images, sample_erase_box
    O = hip.AUG_OPS
    S, T = 32, 2
    imgs = _images()
    crop_boxes = _boxes(4)
    aug_ops = np.array([[O["Rotate"], O["Sharpness"]], [O["ShearX"], O["ShearX"]], [-1, O["Brightness"]], [O["TranslateY"], -1], [-1, -1]], dtype=np.int32)
    erase = [sample_erase_box(S, S, 16, rng=np.random.RandomState(20 + b)) for b in range(5)]
    aug = RandomAugment(2, 7, isPIL=True, augs=["Identity", "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"])
    out = prepare_pretrain_images(imgs, MEAN, STD, crop_size=S, num_frm=T, augment=aug, crop_boxes=crop_boxes, flips=FLIPS, aug_ops=aug_ops, boxes=erase)
    # by hand: the resized crop, the existing augmenter's stages with the same codes, the repeat, the clips' entry point with the same erase boxes
    packed, sizes = _packed()
    rc = hip.resized_crop(packed, sizes, crop_boxes, FLIPS, S)
    assert torch.equal(rc, torch.from_numpy(_expected(S, 4).copy()).cuda())
    staged = TemporalConsistentRandomAugment(N=2, M=7)(rc, ops=aug_ops)
    want = prepare_pretrain_clips(staged.repeat(1, T, 1, 1, 1), MEAN, STD, boxes=erase)
    assert out["visual_inputs"].shape == (5, T, 3, S, S) and out["visual_inputs"].dtype == torch.float32
    for k in ("visual_inputs", "crop_visual_inputs", "context_visual_inputs", "mpm_mask"):
        assert torch.equal(out[k], want[k]), k
        if k != "mpm_mask":
            assert torch.equal(out[k][:, 0], out[k][:, 1]), k                     # a static clip: all frames of an image are equal
    assert out["boxes"] == erase and out["crop_boxes"] == crop_boxes and out["flips"] == FLIPS and np.array_equal(out["aug_ops"], aug_ops)
    assert sorted(out) == sorted(list(want) + ["crop_boxes", "flips", "aug_ops"])
    # everything drawn from the generator, then replayed from what the call returned
    drawn = prepare_pretrain_images(imgs, MEAN, STD, crop_size=S, num_frm=T, augment=aug, rng=np.random.RandomState(3))
    assert len(drawn["crop_boxes"]) == 5 and len(drawn["flips"]) == 5 and drawn["aug_ops"].shape == (5, 2)
    again = prepare_pretrain_images((packed, sizes), MEAN, STD, crop_size=S, num_frm=T, augment=aug, crop_boxes=drawn["crop_boxes"], flips=drawn["flips"],
                                    aug_ops=drawn["aug_ops"], boxes=drawn["boxes"])
    for k in ("visual_inputs", "crop_visual_inputs", "context_visual_inputs", "mpm_mask"):
        assert torch.equal(again[k], drawn[k]), k
    # augment=None: the resized crop and the flip only
    plain = prepare_pretrain_images(imgs, MEAN, STD, crop_size=S, num_frm=T, crop_boxes=crop_boxes, flips=FLIPS, boxes=erase)
    bare = prepare_pretrain_clips(rc.repeat(1, T, 1, 1, 1), MEAN, STD, boxes=erase)
    assert plain["aug_ops"] is None
    for k in ("visual_inputs", "crop_visual_inputs", "context_visual_inputs", "mpm_mask"):
        assert torch.equal(plain[k], bare[k]), k


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_value_and_launch_nothing():
    from alpro_amd import hip
    from alpro_amd.input_gpu import pack_images, prepare_pretrain_images
    packed, sizes = _packed()
    boxes = _boxes(0)
    keep = packed.clone()
    dst = torch.full((5, 1, 3, 8, 8), 77, dtype=torch.uint8, device="cuda")
    tmp = torch.full((5 * 300 * 3 * 8,), 78, dtype=torch.uint8, device="cuda")

    def bad(j, box):
        return boxes[:j] + [box] + boxes[j + 1:]
    with pytest.raises(ValueError, match="output size 30 is not a positive multiple of 4"):
        hip.resized_crop(packed, sizes, boxes, FLIPS, 30, tmp=tmp)
    with pytest.raises(ValueError, match=r"box \(top 10, left 0, h 55, w 48\) of image 1 leaves its 64 x 48 image"):
        hip.resized_crop(packed, sizes, bad(1, (10, 0, 55, 48)), FLIPS, 8, dst=dst, tmp=tmp)
    with pytest.raises(ValueError, match=r"box \(top 0, left -1, h 20, w 20\) of image 2 leaves its 20 x 20 image"):
        hip.resized_crop(packed, sizes, bad(2, (0, -1, 20, 20)), FLIPS, 8, dst=dst, tmp=tmp)
    with pytest.raises(ValueError, match=r"box \(top 3, left 4, h 0, w 5\) of image 0 is empty"):
        hip.resized_crop(packed, sizes, bad(0, (3, 4, 0, 5)), FLIPS, 8, dst=dst, tmp=tmp)
    with pytest.raises(RuntimeError, match="needs uint8 pixels, got torch.float32"):
        hip.resized_crop(packed.float(), sizes, boxes, FLIPS, 8, dst=dst, tmp=tmp)
    with pytest.raises(RuntimeError, match="dst .192 bytes at 0x[0-9a-f]+. overlaps the source buffer"):
        hip.resized_crop(packed, sizes[:1], boxes[:1], FLIPS[:1], 8, dst=packed[384:576].view(1, 1, 3, 8, 8), tmp=tmp)
    wide, wsize = pack_images([np.zeros((1, 5000, 3), np.uint8)])
    with pytest.raises(ValueError, match="5000 pixels of image 0 resized to 8 need 2501 taps, above ALPRO_RESAMPLE_MAX_TAPS = 257"):
        hip.resized_crop(wide, wsize, [(0, 0, 1, 5000)], [False], 8, dst=dst[:1], tmp=tmp)
    with pytest.raises(RuntimeError, match="tmp must hold 36000 bytes"):
        hip.resized_crop(packed, sizes, boxes, FLIPS, 8, dst=dst, tmp=tmp[:100])
    with pytest.raises(ValueError, match="add up to 467190 bytes, the packed buffer holds 1000"):
        hip.resized_crop(packed[:1000], sizes, boxes, FLIPS, 8, dst=dst, tmp=tmp)
    with pytest.raises(ValueError, match="output size 30"):
        prepare_pretrain_images((packed, sizes), MEAN, STD, crop_size=30, num_frm=2, rng=np.random.RandomState(0))
    torch.cuda.synchronize()
    assert (dst == 77).all() and (tmp == 78).all() and torch.equal(packed, keep)
