"""Cases for alpro_attn_probs_grad (the gradient w.r.t. the attention probabilities and the Grad-CAM map, which the flash-style backward never
materialises).  Shared by tests/test_attn_probs_grad_gpu.py (GPU) and tests/test_attn_probs_grad_cpu.py (CPU self-check of the builders); not
collected itself, numpy / torch on the CPU only.

A case is a case of tests/attn_probs_cases.py (q | k | v rounded to the operand dtype, key bias, the fp64 softmax) plus a `dctx` (batch*L, H*64)
ROUNDED TO THE OPERAND DTYPE, in two scales: standard normal with grad_scale = 1, and 2^-10 x the SAME normal draws with grad_scale = 2^10 on
the kernel side (what a loss-scaled backward looks like from the kernel: small operands, a power-of-two factor on the result).  Expectations,
fp64:  G64 = grad_scale * <dctx_bhq, v_bhk>,  CAM64 = p64 * max(G64, 0).

The bounds, u = 2^-24; nothing is fitted to the kernel's output.
  G.   The kernel forms the 64-term dot product with the MFMA in fp32 (products exact for 16-bit operands, rounded once for fp32 ones) and
       multiplies by grad_scale once.  A 64-term fp32 dot product in ANY order is within gamma_64 < 65 u of sum_i |dctx_i| |v_i|, the multiply
       adds one relative rounding of the result:
           |G - G64| <= limG = |grad_scale| * 65 u * sum_i |dctx_i| |v_i| + u * |G64|
  P.   limP = attn_probs_cases.bound(case, lse_err): the kernel's P is alpro_attn_probs' value, bit for bit.
  CAM. CAM = fl(P * max(G, 0)), one fp32 multiply.  ReLU is 1-Lipschitz, so |max(G, 0) - max(G64, 0)| <= limG, and with P <= p64 + limP:
           |CAM - CAM64| <= limP * max(G64, 0) + (p64 + limP) * limG + u * (p64 + limP) * (max(G64, 0) + limG)
       (the error of P times the exact ReLU, the kernel's P times the error of the ReLU, the rounding of the product of the two kernel values).
"""
from collections import namedtuple

import numpy as np

from tests import attn_probs_cases as ac

U = ac.U
SMALL = 2.0 ** -10

GradCase = namedtuple("GradCase", "case dctx grad_scale g64 cam64 absdot")


def dctx_rows64(dctx, batch, L, H):
    return dctx.astype(np.float64).reshape(batch, L, H, 64).transpose(0, 2, 1, 3)   # (batch, H, L, 64)


def grad64(case, dctx, grad_scale):
    """-> (G64, sum_i |dctx_i| |v_i|), (batch, H, L, L) fp64 each."""
    d, v = dctx_rows64(dctx, case.batch, case.L, case.H), ac.values64(case.qkv, case.batch, case.L, case.H)
    return grad_scale * (d @ v.transpose(0, 1, 3, 2)), np.abs(d) @ np.abs(v).transpose(0, 1, 3, 2)


def with_dctx(case, small=False):
    """The case plus its dctx: standard normal, or (small) 2^-10 x the same draws with grad_scale = 2^10; rounded to the operand dtype."""
    rng = ac._rng("dctx", case.name)
    x = rng.standard_normal((case.batch * case.L, case.H * 64))
    dctx = ac.round_to(x * SMALL if small else x, case.dtype)
    gs = 1.0 / SMALL if small else 1.0
    g64, absdot = grad64(case, dctx, gs)
    return GradCase(case, dctx, gs, g64, case.p64 * np.maximum(g64, 0.0), absdot)


def bound_grad(gc):
    return abs(gc.grad_scale) * 65.0 * U * gc.absdot + U * np.abs(gc.g64)


def bound_cam(gc, lse_err):
    lim_p, lim_g, relu = ac.bound(gc.case, lse_err), bound_grad(gc), np.maximum(gc.g64, 0.0)
    p = gc.case.p64 + lim_p
    return lim_p * relu + p * lim_g + U * p * (relu + lim_g)


def check_grad(gc, g, what=""):
    """g (batch, H, L, L) fp32 from the device (numpy).  Prints the figures before it asserts; returns the worst error / bound."""
    g = np.asarray(g)
    assert g.dtype == np.float32 and g.shape == gc.g64.shape, (g.dtype, g.shape)
    err, lim = np.abs(g.astype(np.float64) - gc.g64), bound_grad(gc)
    ratio = float((err / np.maximum(lim, 1e-300)).max())
    print("%s%s grad: max |G - G64| %.3e (max |G64| %.3e), worst error / bound %.3f" % (gc.case.name, what, err.max(), np.abs(gc.g64).max(), ratio))
    assert np.isfinite(g).all(), "inf / NaN"
    assert (err <= lim).all(), "error above the bound by %.3e" % (err - lim).max()
    return ratio


def check_cam(gc, cam, lse, what=""):
    cam = np.asarray(cam)
    assert cam.dtype == np.float32 and cam.shape == gc.cam64.shape, (cam.dtype, cam.shape)
    lse_err = np.abs(np.asarray(lse, dtype=np.float64) - gc.case.lse64)
    err, lim = np.abs(cam.astype(np.float64) - gc.cam64), bound_cam(gc, lse_err)
    ratio = float((err / lim).max())
    print("%s%s cam: max |CAM - CAM64| %.3e (max CAM64 %.3e), worst error / bound %.3f" % (gc.case.name, what, err.max(), gc.cam64.max(), ratio))
    assert np.isfinite(cam).all(), "inf / NaN"
    assert cam.min() >= 0.0, "negative Grad-CAM entry %r" % cam.min()
    assert (err <= lim).all(), "error above the bound by %.3e" % (err - lim).max()
    return ratio
