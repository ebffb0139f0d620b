"""CPU: the host side of the attention-gradient / Grad-CAM output -- alpro_attn_probs_grad's ABI surface and argument checks (every check sits in
front of the first HIP call, so placeholder addresses are never read), the self-check of the case builders (tests/attn_probs_grad_cases.py),
and the refusals of the wrapper, of the collector and of text_to_patch_gradcam that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import attn_probs_cases as ac
from tests import attn_probs_grad_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_point_is_exported_and_declared_and_the_abi_number_stays():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    lib = hip.load()
    assert "alpro_attn_probs_grad" in hip.EXPORTS and re.search(r"\bint\s+alpro_attn_probs_grad\s*\(", hdr) and hasattr(lib, "alpro_attn_probs_grad")
    assert "#define ALPRO_HIP_ABI_VERSION 22" in hdr and hip.ABI_VERSION == 22 == lib.alpro_hip_abi_version()   # additive: one new symbol
    assert os.path.exists(os.path.join(ROOT, "alpro_amd", "csrc", "attention_probs_grad.hip"))


def test_bad_arguments_are_refused_with_a_message_and_without_a_device():
    from alpro_amd import hip
    lib = hip.load()
    p = ctypes.c_void_p(4096)
    good = dict(qkv=p, dctx=p, lse=p, kb=None, grad=p, cam=p, dtype=hip.F16, batch=2, L=40, H=2, q0=0, nq=40, k0=0, nk=40)

    def call(**kw):
        a = dict(good, **kw)
        return lib.alpro_attn_probs_grad(a["qkv"], a["dctx"], a["lse"], a["kb"], a["grad"], a["cam"], a["dtype"], a["batch"], a["L"], a["H"], 0.125, 1.0,
                                         a["q0"], a["nq"], a["k0"], a["nk"], None)

    big = hip_max_l() + 1
    for kw, msg in ((dict(dtype=3), "dtype=3"), (dict(dtype=-1), "dtype=-1"),
                    (dict(L=0, nq=0, nk=0), "L=0"), (dict(L=big, nq=big, nk=big), "L=%d" % big),
                    (dict(q0=8, nq=33), "q0=8 nq=33"), (dict(k0=39, nk=2), "k0=39 nk=2"), (dict(q0=-1, nq=3), "q0=-1"), (dict(k0=-2, nk=3), "k0=-2"),
                    (dict(nq=0), "nq=0"), (dict(nk=0), "nk=0"), (dict(k0=2147483647, nk=2), "k0=2147483647"),
                    (dict(grad=None, cam=None), "null grad_out and null cam_out"),
                    (dict(qkv=None), "null qkv"), (dict(dctx=None), "null dctx"), (dict(lse=None), "null lse"),
                    (dict(batch=0), "batch=0"), (dict(H=0), "H=0"),
                    (dict(qkv=ctypes.c_void_p(4096 + 8)), "16-byte aligned"), (dict(dctx=ctypes.c_void_p(4096 + 2)), "16-byte aligned"),
                    (dict(grad=ctypes.c_void_p(4096 + 4)), "16-byte aligned"), (dict(cam=ctypes.c_void_p(4096 + 4), grad=None), "16-byte aligned"),
                    (dict(lse=ctypes.c_void_p(4096 + 2)), "4-byte aligned")):
        rc = call(**kw)
        assert rc != 0, kw
        assert msg in lib.alpro_hip_last_error().decode(), (kw, lib.alpro_hip_last_error())


def hip_max_l():
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    return int(re.search(r"#define ALPRO_ATTN_MAX_L (\d+)", hdr).group(1))


def test_wrapper_refuses_cpu_tensors_and_a_bad_want():
    from alpro_amd import hip
    qkv, dctx, lse = torch.zeros(2 * 8, 3 * 2 * 64), torch.zeros(2 * 8, 2 * 64), torch.zeros(2, 2, 8)
    with pytest.raises(RuntimeError, match="qkv must be a device tensor.*no CPU fallback"):
        hip.attn_probs_grad(qkv, dctx, lse, 2, 8, 2, 0.125)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attn_probs_grad(np.zeros((16, 384), dtype=np.float32), dctx, lse, 2, 8, 2, 0.125)
    for want in ((), ("probs",), ("cam", "cam"), "map"):
        with pytest.raises(RuntimeError, match="want="):
            hip.attn_probs_grad(qkv, dctx, lse, 2, 8, 2, 0.125, want=want)


@pytest.mark.parametrize("dtype", ac.DTYPES)
def test_case_builders_hold_what_they_claim(dtype):
    c = ac.random_case(5, dtype, batch=2, H=2, bias="pad")
    for small in (False, True):
        g = gc.with_dctx(c, small=small)
        assert g.dctx.shape == (2 * 5, 2 * 64) and g.dctx.dtype == np.float32
        assert np.array_equal(ac.round_to(g.dctx, dtype), g.dctx)          # already representable in the operand dtype
        assert g.grad_scale == (1024.0 if small else 1.0)
        # G64 against a plain loop
        qkv = c.qkv.astype(np.float64)
        for b, h, q, k in ((0, 0, 0, 0), (1, 1, 4, 2), (0, 1, 3, 4), (1, 0, 2, 2)):
            want = 0.0
            for i in range(64):
                want += float(g.dctx[b * 5 + q, h * 64 + i]) * float(qkv[b * 5 + k, 2 * 2 * 64 + h * 64 + i])
            assert abs(g.g64[b, h, q, k] - g.grad_scale * want) <= 1e-12 * max(1.0, abs(want) * g.grad_scale)
        assert np.array_equal(g.cam64, c.p64 * np.maximum(g.g64, 0.0)) and (g.cam64 >= 0).all() and (g.g64 < 0).any() and (g.g64 > 0).any()
        lim_g, lim_c = gc.bound_grad(g), gc.bound_cam(g, np.zeros_like(c.lse64))
        assert np.isfinite(lim_g).all() and (lim_g > 0).all() and np.isfinite(lim_c).all() and (lim_c > 0).all()
        assert (lim_g <= 1e-4 * max(1.0, np.abs(g.g64).max())).all()      # a bound, not a blank cheque
        # check_* accept the fp64 answer rounded to fp32 and refuse a transposed map and a sign flip
        g32, cam32, lse32 = g.g64.astype(np.float32), g.cam64.astype(np.float32), c.lse64.astype(np.float32)
        gc.check_grad(g, g32)
        gc.check_cam(g, cam32, lse32)
        with pytest.raises(AssertionError):
            gc.check_grad(g, np.ascontiguousarray(g32.transpose(0, 1, 3, 2)))
        with pytest.raises(AssertionError):
            gc.check_cam(g, (c.p64 * np.maximum(-g.g64, 0.0)).astype(np.float32), lse32)
    # the two scales are the same draws: unscaled G64 == scaled G64 where the small dctx needed no second rounding (fp32, bf16: same exponent range)
    a, b = gc.with_dctx(c, small=False), gc.with_dctx(c, small=True)
    if dtype != "fp16":
        assert np.array_equal(a.dctx * np.float32(gc.SMALL), b.dctx) and np.abs(a.g64 - b.g64).max() <= 1e-12 * np.abs(a.g64).max()


def test_with_a_non_negative_gradient_the_cam_is_p_times_g():
    c = ac.random_case(5, "fp32", batch=2, H=2, bias="none")
    g = gc.with_dctx(c)
    # make every dot product non-negative: dctx := |dctx|, v := |v|
    qkv = c.qkv.copy()
    qkv[:, 2 * 2 * 64:] = np.abs(qkv[:, 2 * 2 * 64:])
    c2 = c._replace(qkv=qkv)
    g64, _ = gc.grad64(c2, np.abs(g.dctx), 1.0)
    assert (g64 >= 0).all()
    assert np.array_equal(c.p64 * np.maximum(g64, 0.0), c.p64 * g64)


def test_collector_validates_its_arguments_and_refuses_an_early_read():
    from alpro_amd.modeling.xbert import AttnGradients
    with pytest.raises(ValueError, match="want="):
        AttnGradients(want=("probs",))
    with pytest.raises(ValueError, match="no layer chosen"):
        AttnGradients(layers=())
    with pytest.raises(ValueError, match="grad_scale"):
        AttnGradients(grad_scale=0.0)
    col = AttnGradients(layers=(-1, 0), want=("grad", "cam"))
    with pytest.raises(RuntimeError, match="not passed to"):
        col.grads
    with pytest.raises(ValueError, match="layer 2 outside the 2 layers"):
        AttnGradients(layers=(2,)).begin(2)
    col.begin(3)
    assert col.wants(0) and col.wants(2) and not col.wants(1) and col.first() == 0
    with pytest.raises(RuntimeError, match=r"backward\(\) has not run"):
        col.cams
    only = AttnGradients(want="cam")
    only.begin(1)
    only._pending.clear()
    with pytest.raises(RuntimeError, match="want="):
        only.grads
    assert only.cams == {}


def test_text_to_patch_gradcam_refuses_train_mode_a_ragged_grid_and_a_scale_that_is_no_power_of_two():
    from alpro_amd.grounding import text_to_patch_gradcam
    m = torch.nn.Module().train()
    ids = torch.zeros(2, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
        text_to_patch_gradcam(m, ids, torch.ones_like(ids), torch.zeros(2, 5, 64))
    with pytest.raises(ValueError, match="square patch grid"):
        text_to_patch_gradcam(m.eval(), ids, torch.ones_like(ids), torch.zeros(2, 7, 64))
    with pytest.raises(ValueError, match="power of two"):
        text_to_patch_gradcam(m.eval(), ids, torch.ones_like(ids), torch.zeros(2, 5, 64), grad_scale=3.0)
