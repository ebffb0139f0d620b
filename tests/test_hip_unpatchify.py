"""GPU: alpro_unpatchify (csrc/unpatchify.hip), the inverse data movement of alpro_patchify, bit for bit with ZERO tolerance on the shapes of
the patchify cases x fp32 / fp16 / bf16 rows (tests/pixel_grad_cases.py): against F.fold, with the image inside a sentinel-filled buffer whose
guard elements must keep their bits and the rows inside a NaN-filled one; unpatchify(patchify(img)) == img; two runs equal."""
import pytest
import torch

from tests import movement_cases as mc
from tests import pixel_grad_cases as pc
from tests.gemm_cases import DT_NAME, F32, SENTINEL, poisoned
from tests.test_hip_movement_exact import _hip, assert_same

pytestmark = pytest.mark.gpu
G = mc.GUARD
IDS = ["x".join(map(str, s)) for s in pc.SHAPES]


@pytest.mark.parametrize("dt", mc.DTS, ids=[DT_NAME[d] for d in mc.DTS])
@pytest.mark.parametrize("shape", pc.SHAPES, ids=IDS)
def test_unpatchify_exact(shape, dt):
    hip = _hip()
    BT, C, H, W = shape
    rows = pc.unpatchify_rows(shape, dt)
    ref = pc.unpatchify_ref(rows, BT, C, H, W)
    src = poisoned(rows, G, 0, G, device="cuda")            # G NaN rows before and behind (a row is C * 256 elements: every row start stays 16-byte aligned)
    assert src.is_contiguous() and src.data_ptr() % 16 == 0
    got = hip.unpatchify(src, BT, C, H, W)
    assert got.dtype == F32 and tuple(got.shape) == shape
    assert_same(got.view(-1, W), ref.view(-1, W), "unpatchify (wrapper) %s" % (shape,))
    # through the C entry point into a sentinel-filled buffer: G guard image rows on either side of the BT * C * H image rows
    want = poisoned(ref.view(-1, W), G, 0, G, fill=SENTINEL)
    buf = torch.full(tuple(want._base.shape), SENTINEL, dtype=F32, device="cuda")
    out = buf[G:G + BT * C * H]
    assert out.data_ptr() % 16 == 0
    hip._check(hip.load().alpro_unpatchify(hip._ptr(src), hip.dtype_code(dt), hip._ptr(out), BT, C, H, W, hip._stream()), "alpro_unpatchify")
    assert_same(buf, want._base, "unpatchify buffer %s" % (shape,))
    # out=: a caller's buffer of another shape (the model hands a (B, T, C, H, W) one), and a second run
    again = torch.full((BT * C, H * W), SENTINEL, dtype=F32, device="cuda")
    assert hip.unpatchify(src, BT, C, H, W, out=again) is again
    assert torch.equal(again.view(shape), got), "two runs differ"


@pytest.mark.parametrize("shape", pc.SHAPES, ids=IDS)
def test_unpatchify_inverts_patchify(shape):
    hip = _hip()
    BT, C, H, W = shape
    img = mc.patchify_image(shape, F32).cuda()
    back = hip.unpatchify(hip.patchify(img, F32), BT, C, H, W)
    assert_same(back.view(-1, W), img.view(-1, W), "unpatchify(patchify(img))")
    # and the other way round, through 16-bit rows
    for dt in mc.DTS[1:]:
        rows = pc.unpatchify_rows(shape, dt).cuda()
        assert_same(hip.patchify(hip.unpatchify(rows, BT, C, H, W), dt), rows, "patchify(unpatchify(rows)) %s" % DT_NAME[dt])


def test_wrapper_refusals_on_the_device():
    hip = _hip()
    rows = torch.zeros(2 * 4, 768, device="cuda")
    with pytest.raises(ValueError, match="expected a contiguous"):
        hip.unpatchify(rows, 2, 3, 32, 64)
    with pytest.raises(ValueError, match="multiple of the 16x16 patch"):
        hip.unpatchify(rows, 2, 3, 32, 24)
    with pytest.raises(RuntimeError, match="fp32, fp16 or bf16"):
        hip.unpatchify(rows.double(), 2, 3, 32, 32)
    with pytest.raises(ValueError, match="out must be"):
        hip.unpatchify(rows, 2, 3, 32, 32, out=torch.zeros(2, 3, 32, 16, device="cuda"))
    with pytest.raises(RuntimeError, match="expected torch.float32"):
        hip.unpatchify(rows, 2, 3, 32, 32, out=torch.zeros(2, 3, 32, 32, device="cuda", dtype=torch.float16))
