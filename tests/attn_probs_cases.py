"""Cases for alpro_attn_probs (the attention probabilities the flash-style forward never materialises).  Shared by tests/test_attn_probs_gpu.py
(GPU) and tests/test_attn_probs_cpu.py (CPU self-check of the builders); not collected itself, numpy / torch on the CPU only.

A case is q | k | v rows ROUNDED TO THE OPERAND DTYPE first (so the fp64 expectation and the kernel read the same numbers), an optional additive
key bias, and the fp64 softmax of scale * q k^T + bias with its log-sum-exp.

The bound.  The kernel computes p = exp2(log2(e) * min(fl(fl(scale * acc + bias) - lse), 0)) with acc the MFMA's 64-term fp32 dot product.
Against p64 = exp(s64 - lse64) the argument is off by at most
    d = 65 * 2^-24 * scale * sum_i |q_i| |k_i|      worst case of a 64-term fp32 dot product in any order (gamma_64 < 65 u, u = 2^-24; 0 for 16-bit
                                                    operands would also hold -- their products are exact in fp32 -- but the sums still round)
      + 2^-24 * (|s64| + the line above)            the ONE fp32 rounding of s = fma(acc, scale, bias) (scale = 1/8 is a power of two)
      + |lse - lse64|                               the OBSERVED error of the forward kernel's log-sum-exp row (an input of alpro_attn_probs)
so |p - p64| <= p64 * (exp(d) - 1) + 2^-23.  The absolute term covers what is left, all of it proportional to p |ln p| <= 1/e or to one ulp of
a result below 1: the rounding of the subtraction (u |a|, a = s - lse), of the multiply by log2(e) and of that constant (1.5 u |a|), and the
hardware exponential's 1 ulp (v_exp_f32, CDNA ISA guide: <= 2^-24 absolute for results below 1): p (2.5 u |ln p|) + 2^-24 <= 1.92 * 2^-24 <
2^-23; it also covers results flushed to zero below 2^-126 and the clamp at 1.  Nothing here is fitted to the kernel's output.
"""
import zlib
from collections import namedtuple

import numpy as np
import torch

LENGTHS = (1, 31, 32, 33, 64, 65, 237, 257, 300)   # tile edges of the 32-key / 32-query tiles, the fusion length, both sides of L = 256
DTYPES = ("fp32", "bf16", "fp16")
TORCH_DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SCALE = 0.125                                      # 1 / sqrt(head_dim 64)
U = 2.0 ** -24

Case = namedtuple("Case", "name batch L H dtype scale qkv bias s64 p64 lse64 absdot")


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def round_to(x, dtype):
    """fp32 numpy array -> the same values rounded to the operand dtype (round-to-nearest-even, torch's conversion), back in fp32."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TORCH_DTYPE[dtype]).to(torch.float32).numpy()


def key_bias(kind, batch, L):
    """(batch, L) fp32 additive key bias as BertModel.key_bias builds it, or None.  'mixed': sequence 0 masks its trailing keys, sequence 1 one
    middle key, sequence 2 (and every third one) ALL keys -- the constant cancels in the softmax, but every s sits at -10000, where fp32 resolves 2^-10.
    'pad': the same without the all-masked sequence (every score that matters stays of order 1)."""
    if kind == "none":
        return None
    assert kind in ("mixed", "pad")
    m = np.ones((batch, L), dtype=np.float32)
    for b in range(batch):
        if b % 3 == 0:
            m[b, L - max(1, L // 4):] = 0
        elif b % 3 == 1:
            m[b, L // 2] = 0
        elif kind == "mixed":
            m[b, :] = 0
    return ((1.0 - m) * np.float32(-10000.0)).astype(np.float32)


def softmax64(qkv, bias, batch, L, H, scale):
    """-> (s64, p64, lse64, absdot): scores, softmax, log-sum-exp and sum_i |q_i| |k_i| in fp64, (batch, H, L, L) / (batch, H, L)."""
    x = qkv.astype(np.float64).reshape(batch, L, 3, H, 64)
    q, k = x[:, :, 0].transpose(0, 2, 1, 3), x[:, :, 1].transpose(0, 2, 1, 3)      # (batch, H, L, 64)
    s = scale * (q @ k.transpose(0, 1, 3, 2))
    absdot = np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2)
    if bias is not None:
        s = s + bias.astype(np.float64)[:, None, None, :]
    m = s.max(axis=-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(s - m).sum(axis=-1))
    return s, np.exp(s - lse[..., None]), lse, absdot


def values64(qkv, batch, L, H):
    return qkv.astype(np.float64).reshape(batch, L, 3, H, 64)[:, :, 2].transpose(0, 2, 1, 3)   # (batch, H, L, 64)


def random_case(L, dtype, batch=3, H=2, bias="mixed"):
    rng = _rng("probs", L, dtype, batch, H, bias)
    qkv = round_to(rng.standard_normal((batch * L, 3 * H * 64)), dtype)   # s = q . k / 8 has unit variance: rows with a few dominant keys
    kb = key_bias(bias, batch, L)
    s, p, lse, ad = softmax64(qkv, kb, batch, L, H, SCALE)
    return Case("L%d_%s_B%d_H%d_%s" % (L, dtype, batch, H, bias), batch, L, H, dtype, SCALE, qkv, kb, s, p, lse, ad)


def peaked_case(L, dtype, batch=2, H=2):
    """|s| of about 60: every key is +-c times one sign pattern and every query +-c times the same pattern (c^2 * 64 / 8 = 60), plus noise, so a
    row has keys at +60 beside keys at -60: exp(-120) next to probabilities that sum to 1 over the aligned keys."""
    rng = _rng("peaked", L, dtype, batch, H)
    c = np.sqrt(60.0 * 8.0 / 64.0)
    pat = np.where(rng.rand(64) < 0.5, -1.0, 1.0)
    x = 0.05 * rng.standard_normal((batch, L, 3, H, 64))
    sq, sk = np.where(rng.rand(batch, L, H) < 0.5, -1.0, 1.0), np.where(rng.rand(batch, L, H) < 0.5, -1.0, 1.0)
    x[:, :, 0] += c * sq[..., None] * pat
    x[:, :, 1] += c * sk[..., None] * pat
    qkv = round_to(x.reshape(batch * L, 3 * H * 64), dtype)
    s, p, lse, ad = softmax64(qkv, None, batch, L, H, SCALE)
    return Case("peaked_L%d_%s" % (L, dtype), batch, L, H, dtype, SCALE, qkv, None, s, p, lse, ad)


def bound(case, lse_err):
    """Per-element limit on |p - p64| (module docstring); lse_err (batch, H, L) = |lse - lse64| observed on the forward kernel's rows."""
    dot = 65.0 * U * case.scale * case.absdot
    d = dot + U * (np.abs(case.s64) + dot) + np.asarray(lse_err, dtype=np.float64)[..., None]
    return case.p64 * np.expm1(d) + 2.0 ** -23


def check(case, p, lse, what=""):
    """p (batch, H, L, L) fp32 and lse (batch, H, L) fp32 from the device (numpy): inside the bound, in [0, 1], rows sum to 1 within the bound's
    row sum.  Prints the figures before it asserts.  Returns (max error, max of error / bound)."""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.shape == case.p64.shape, (p.dtype, p.shape)
    lse_err = np.abs(np.asarray(lse, dtype=np.float64) - case.lse64)
    lim = bound(case, lse_err)
    err = np.abs(p.astype(np.float64) - case.p64)
    rows = np.abs(p.astype(np.float64).sum(axis=-1) - 1.0)
    row_lim = lim.sum(axis=-1) + 1e-12   # (+ the fp64 reference's own rounding of a row sum)
    print("%s%s: max |p - p64| %.3e, worst error / bound %.3f, max |lse - lse64| %.3e, worst |row sum - 1| %.3e (its bound %.3e)"
          % (case.name, what, err.max(), (err / lim).max(), lse_err.max(), rows.max(), row_lim[np.unravel_index(rows.argmax(), rows.shape)]))
    assert np.isfinite(p).all(), "inf / NaN"
    assert p.min() >= 0.0 and p.max() <= 1.0, "outside [0, 1]: min %r max %r" % (p.min(), p.max())
    assert (err <= lim).all(), "error above the bound by %.3e" % (err - lim).max()
    assert (rows <= row_lim).all(), "row sums off by %.3e" % (rows - row_lim).max()
    return float(err.max()), float((err / lim).max())
