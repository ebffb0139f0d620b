"""CPU: the host side of the pixel gradient -- the case builders of tests/pixel_grad_cases.py against an explicit loop, alpro_unpatchify's ABI
surface and argument checks (every check sits in front of the first HIP call, so placeholder addresses are never read), the refusals of
hip.unpatchify and of the two grounding helpers that need no device, and the fp64 oracle's pixel gradient against the reference's own
(tests/golden/vit_pixel_grad_*.npz) within the tolerance tests/test_oracle_golden.py applies to gradients (rtol 2e-3, atol 2e-6)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pixel_grad_cases as pc
from tests.conftest import GOLDEN
from tests.gemm_cases import BF16, F16, F32, F64
from tests.golden.make_golden_pixel_grad import MODES, fixture_name, out_modes
from tests.golden.make_golden_pool_modes import GEOMETRIES
from tests.movement_cases import patchify_image, patchify_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", pc.SHAPES, ids=["x".join(map(str, s)) for s in pc.SHAPES])
def test_builders_against_an_explicit_loop(shape):
    BT, C, H, W = shape
    gw, N = W // 16, (H // 16) * (W // 16)
    for dt in (F32, BF16, F16):
        rows = pc.unpatchify_rows(shape, dt)
        assert tuple(rows.shape) == pc.rows_shape(shape) == (BT * N, C * 256) and rows.dtype == dt
        ref = pc.unpatchify_ref(rows, BT, C, H, W)
        assert ref.dtype == F32 and tuple(ref.shape) == shape
        r64 = rows.to(F64)
        for bt in range(BT):
            for c in range(C):
                for y in range(0, H, 5):
                    for x in range(0, W, 3):
                        want = r64[bt * N + (y // 16) * gw + x // 16, c * 256 + (y % 16) * 16 + x % 16]
                        assert float(ref[bt, c, y, x]) == float(want), (bt, c, y, x)
        # neighbours differ in every direction (a shifted or transposed write cannot pass), and the rows invert patchify's reference
        assert bool((ref[..., 1:] != ref[..., :-1]).all()) and (H == 16 or bool((ref[:, :, 1:] != ref[:, :, :-1]).all()))
        assert torch.equal(patchify_ref(ref), r64)
    img = patchify_image(shape, F32)
    assert torch.equal(pc.unpatchify_ref(patchify_ref(img), BT, C, H, W), img)
    assert torch.equal(F.fold(F.unfold(img, 16, stride=16), (H, W), 16, stride=16), img)


def test_new_entry_point_is_exported_and_declared_and_the_abi_number_stays():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    lib = hip.load()
    assert "alpro_unpatchify" in hip.EXPORTS and re.search(r"\bint\s+alpro_unpatchify\s*\(", hdr) and hasattr(lib, "alpro_unpatchify")
    assert "#define ALPRO_HIP_ABI_VERSION 22" in hdr and hip.ABI_VERSION == 22 == lib.alpro_hip_abi_version()   # additive: one new symbol
    assert os.path.exists(os.path.join(ROOT, "alpro_amd", "csrc", "unpatchify.hip"))
    assert callable(hip.unpatchify)


def test_bad_arguments_are_refused_with_a_message_and_without_a_device():
    from alpro_amd import hip
    lib = hip.load()
    p = ctypes.c_void_p(4096)
    good = dict(rows=p, dtype=hip.F16, img=p, BT=2, C=3, H=32, W=48)

    def call(**kw):
        a = dict(good, **kw)
        return lib.alpro_unpatchify(a["rows"], a["dtype"], a["img"], a["BT"], a["C"], a["H"], a["W"], None)

    for kw, msg in ((dict(rows=None), "null rows"), (dict(img=None), "null img"), (dict(BT=0), "BT=0"), (dict(BT=-1), "BT=-1"), (dict(C=0), "C=0"),
                    (dict(C=-3), "C=-3"), (dict(H=24), "image 24x48 not a multiple"), (dict(W=40), "image 32x40 not a multiple"),
                    (dict(H=0), "image 0x48"), (dict(W=-16), "image 32x-16"), (dict(dtype=3), "dtype=3"), (dict(dtype=-1), "dtype=-1"),
                    (dict(rows=ctypes.c_void_p(4096 + 8)), "16-byte aligned"), (dict(img=ctypes.c_void_p(4096 + 4)), "16-byte aligned"),
                    (dict(BT=2 ** 31 - 1, H=16 * 1024, W=16 * 1024), "more than 2^31 - 1")):
        assert call(**kw) != 0, kw
        assert msg in lib.alpro_hip_last_error().decode(), (kw, lib.alpro_hip_last_error())


def test_wrapper_refuses_cpu_tensors():
    from alpro_amd import hip
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.unpatchify(torch.zeros(4, 768), 1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.unpatchify(torch.zeros(4, 768, dtype=torch.float16), 1, 3, 32, 32, out=torch.zeros(1, 3, 32, 32))


def test_grounding_helpers_refuse_on_the_host():
    from alpro_amd.grounding import pixel_gradient, text_to_pixel_saliency
    m = torch.nn.Module().train()
    ids = torch.zeros(2, 8, dtype=torch.long)
    mask, clip = torch.ones_like(ids), torch.zeros(2, 2, 3, 32, 32)
    for fn in (pixel_gradient, text_to_pixel_saliency):
        with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
            fn(m.train(), ids, mask, clip)
        m.eval()
        with pytest.raises(ValueError, match=r"not \(B, T, C, H, W\)"):
            fn(m, ids, mask, clip[0])
        with pytest.raises(ValueError, match="multiples of the 16-pixel patch"):
            fn(m, ids, mask, torch.zeros(2, 2, 3, 32, 24))
        with pytest.raises(ValueError, match="one caption per clip"):
            fn(m, ids[:1], mask[:1], clip)
        with pytest.raises(ValueError, match="one caption per clip"):
            fn(m, ids, mask[:, :7], clip)
        for bad in (3.0, 0.0, -2.0, float("inf")):
            with pytest.raises(ValueError, match="power of two"):
                fn(m, ids, mask, clip, grad_scale=bad)
    for bad in ("gradcam", "", None):
        with pytest.raises(ValueError, match="method="):
            text_to_pixel_saliency(m.train(), ids, mask, clip, method=bad)   # before anything else: not even the mode is looked at


@pytest.mark.parametrize("geo", range(len(GEOMETRIES)))
def test_oracle_pixel_gradient_reproduces_the_reference(geo):
    g = np.load(os.path.join(GOLDEN, fixture_name(GEOMETRIES[geo])))
    _, x, ref = pc.oracle_case(geo)
    assert np.array_equal(g["x"].astype(np.float32), x.numpy())
    for mode in MODES:
        out, dx = ref[mode]
        if mode in out_modes(GEOMETRIES[geo]):
            np.testing.assert_allclose(out.numpy(), g[mode + "/out"].astype(np.float64), rtol=2e-4, atol=2e-5, err_msg=mode + " out")
        want = g[mode + "/dx"].astype(np.float64)
        assert dx.shape == x.shape
        print("\n[oracle pixel gradient img%d %s] max |dx| %.3e, max err %.3e" % (GEOMETRIES[geo]["img"], mode, np.abs(want).max(), np.abs(dx.numpy() - want).max()))
        np.testing.assert_allclose(dx.numpy(), want, rtol=2e-3, atol=2e-6, err_msg=mode + " dx")
