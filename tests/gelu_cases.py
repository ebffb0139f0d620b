"""Range and accuracy cases for the GELU family: the six hand-written forms of csrc/common.hpp on every route that reaches them (alpro_gemm's
three kernels with ACT_GELU / ACT_GELU_SAVE_GRAD / ACT_GELU_BWD, alpro_gelu_bwd, alpro_gemm_rows_f32).  Shared by tests/test_hip_gelu_range.py
(GPU) and tests/test_gelu_cases_cpu.py (CPU self-check); not collected itself, torch and numpy on the CPU only.

The idea: the kernel must see the exact fp32 pre-activation x the reference sees, so the weights only SELECT -- one or two ones per row of W,
alpha a power of two -- and the fp32 accumulator is exact in every summation order:
  (a) "every16": A (256, 256) holds all 65536 bit patterns of a 16-bit dtype (non-finite ones replaced by 0), W is the identity: pre = A, bit
      for bit -- subnormals, +-0 and the whole finite range (bf16 to 3.4e38, fp16 to 65504; fp16 again times alpha = 2^16);
  (b) "grid": x = k 2^-12 for every k in [-2^15, 2^15) ([-8, 8)) and x = +-(8 + k 2^-11), k in [0, 2^14) (to +-16), each split into two
      operand-dtype pieces hi + lo in columns 2n, 2n + 1 of A with W[n, 2n] = W[n, 2n + 1] = 1: the fp32 points between the 16-bit ones;
  (c) "far": A = 0, so pre[m, n] = bias[n]: +-2^k for k = 4 .. 127, +-7e4, +-7.5e4, +-1e5, +-1e10, +-3e38, the smallest normal and a subnormal
      fp32; NaN, +inf and -inf in a launch of their own.

The condition (no blanket rtol / atol).  The reference is fp64 with Phi(x) = 0.5 erfc(-x / sqrt 2), which keeps the digits of the negative
tail (1 + erf does not).  For a form whose Phi is within E of the truth,
    tol_y(x)  = E |x| + 4 2^-24 |gelu(x)| + 2^-126              tol_dy(x) = E + 4 2^-24 (1 + |x| phi(x)) + 2^-126
and an output of dtype D must lie in the closed interval [rn_D(ref - tol), rn_D(ref + tol)], rn_D = round to nearest-even into D (the
identity for fp32): a misrounding, a second rounding or a pre-activation rounded to 16 bits before the GELU falls outside.  E comes from the
comments of common.hpp: E_2Q for the erfc ~= 2^q(z) forms (half of the stated 6.8e-7 on erfc), E_PAIR for gelu_and_grad2; the libm forms
(erff / __expf: the fp32 operand mode, alpro_gelu_bwd, alpro_gemm_rows_f32) have E_LIBM, twice what was measured on an MI355X and never above
8 2^-24.
"""
import math

import torch

from tests.gemm_cases import ACT_GELU, ACT_GELU_SAVE_GRAD, BF16, DT_NAME, F16, F32, F64   # noqa: F401  (re-exported)

U24 = 2.0 ** -24
TINY = 2.0 ** -126
E_2Q = 3.4e-7            # gelu_fast, gelu_fast2, gelu_grad<T>, gelu_and_grad<T> for 16-bit T
E_PAIR = 3.2e-7          # gelu_and_grad2
E_LIBM_CAP = 8.0 * U24
# Worst |Phi error| of the libm forms measured on an MI355X against fp64, in units of 2^-24: 1.83, seen through y / x (so including the one
# rounding of y) of alpro_gemm's fp32 mode on all three routes and of alpro_gemm_rows_f32 on grid (b); alpro_gelu_bwd's gelu' is within 2.13.
# tests/test_hip_gelu_range.py prints the figure on every run.  Asserted at twice the measured value: 3.66 x 2^-24 = 2.18e-7.
E_LIBM_MEASURED_U24 = 1.83
E_LIBM = min(2.0 * E_LIBM_MEASURED_U24 * U24, E_LIBM_CAP)
SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794


# ------------------------------------------------------------------------------------------------ reference and condition
def Phi64(x):
    return 0.5 * torch.special.erfc(-x.to(F64) / math.sqrt(2.0))


def phi64(x):
    x = x.to(F64)
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu64(x, fault=None):
    """fault: "tanh" = the tanh-form GELU in place of the erf form."""
    x = x.to(F64)
    if fault == "tanh":
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return torch.where(x == 0, x, x * Phi64(x))      # (keeps inf * 0 out of the far values: Phi64(-3e38) = 0 and x finite there anyway)


def gelu_grad64(x, fault=None):
    """fault: "no_x_phi" = gelu' without its x phi(x) term."""
    x = x.to(F64)
    if fault == "no_x_phi":
        return Phi64(x)
    return Phi64(x) + x * phi64(x)


def tol_y(x, E):
    x = x.to(F64)
    return E * x.abs() + 4.0 * U24 * gelu64(x).abs() + TINY


def tol_dy(x, E):
    x = x.to(F64)
    return E + 4.0 * U24 * (1.0 + x.abs() * phi64(x)) + TINY


def interval(ref, tol, dt, factor=None):
    """-> (lo, hi) fp64: [rn_dt((ref - tol) f), rn_dt((ref + tol) f)] ordered, f the exact factor of a GELU_BWD output (None = 1)."""
    a, b = ref - tol, ref + tol
    if factor is not None:
        a, b = a * factor, b * factor
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    if dt != F32:      # (fp32: the identity -- the sums above are fp64 and an fp32 value inside [lo, hi] is inside)
        lo, hi = lo.to(dt).to(F64), hi.to(dt).to(F64)
    return lo, hi


def outside(got, x, ref, tol, dt, factor=None):
    """Boolean mask of the elements of `got` (a tensor of dtype dt, any device) that miss the interval; NaN misses it."""
    lo, hi = interval(ref, tol, dt, factor)
    g = got.detach().cpu().to(F64)
    return ~((g >= lo) & (g <= hi))


def worst_ratio(got, ref, tol, factor=None):
    """max |got - ref| / tol: the margin a reader sees (meaningful for fp32 outputs; a 16-bit output adds its rounding)."""
    g = got.detach().cpu().to(F64)
    f = 1.0 if factor is None else factor
    r = ((g - ref * f).abs() / (tol * (f.abs() if torch.is_tensor(f) else abs(f)))).nan_to_num(nan=float("inf"))
    return float(r.max())


def must_be_finite(x, ref, dt):
    """Where a finite input must give a finite output: everywhere the correctly rounded reference is finite (an fp16 output overflows
    legitimately beyond 65504)."""
    return x.isfinite() & ref.to(dt).isfinite()


# ------------------------------------------------------------------------------------------------ the pre-activations
_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def every16(dt):
    """(256, 256) of dt: all 65536 bit patterns, the non-finite ones replaced by 0."""
    def make():
        v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt).view(256, 256).clone()
        v[~v.isfinite()] = 0
        return v
    return _cached(("every16", dt), make)


GRID_ROWS = 384


def grid_points():
    """(384, 256) fp64: [-8, 8) in steps of 2^-12 (256 rows), then +(8 + k 2^-11) and -(8 + k 2^-11), k in [0, 2^14) (64 rows each: to +-16)."""
    def make():
        k = torch.arange(-2 ** 15, 2 ** 15, dtype=F64)
        j = torch.arange(0, 2 ** 14, dtype=F64)
        far = 8.0 + j * 2.0 ** -11
        return torch.cat([k * 2.0 ** -12, far, -far]).view(GRID_ROWS, 256)
    return _cached("grid", make)


def split_hi_lo(x, dt):
    """x (fp64) -> hi, lo of dt with hi + lo == x (for fp32: lo = 0)."""
    hi = x.to(dt)
    lo = (x - hi.to(F64)).to(dt)
    return hi, lo


FAR_M, FAR_N, FAR_K = 256, 512, 256
F16_ALPHA = 2.0 ** 16
NONFINITE = (float("nan"), float("inf"), float("-inf"))


def every_case(dt, val_dt=None):
    """(a): (256, 256, 256), A = every value of val_dt (the operand dtype; bf16 or fp16 values, exact in fp32, for fp32 operands), W = I."""
    val_dt = val_dt or dt

    def make():
        ev = every16(val_dt)
        a = ev.to(dt)
        assert torch.equal(a.to(F64), ev.to(F64))
        return dict(a=a, w=torch.eye(256, dtype=dt), bias=None, alpha=1.0, pre=ev.to(F64))
    return _cached(("every", dt, val_dt), make)


def grid_case(dt):
    """(b): (512, 256, 512) -- 384 rows of grid points as hi + lo in columns 2n, 2n + 1, zero rows up to two whole 256-row tiles (every
    wave of every route then takes its full-tile path, the one the route is named for)."""
    def make():
        gp = grid_points()
        hi, lo = split_hi_lo(gp, dt)
        a = torch.zeros(512, 512, dtype=dt)
        a[:GRID_ROWS, 0::2], a[:GRID_ROWS, 1::2] = hi, lo
        pre = torch.zeros(512, 256, dtype=F64)
        pre[:GRID_ROWS] = gp
        w = torch.zeros(256, 512, dtype=dt)
        n = torch.arange(256)
        w[n, 2 * n] = 1
        w[n, 2 * n + 1] = 1
        return dict(a=a, w=w, bias=None, alpha=1.0, pre=pre)
    return _cached(("grid", dt), make)


def far_values():
    """(512,) fp32, the bias of (c): the finite far values, zero-padded."""
    def make():
        p = [2.0 ** k for k in range(4, 128)]
        v = p + [-t for t in p]
        for t in (7e4, 7.5e4, 1e5, 1e10, 3e38):
            v += [t, -t]
        v += [2.0 ** -126, -2.0 ** -126, 2.0 ** -140, -2.0 ** -140, 2.0 ** -149]
        b = torch.zeros(FAR_N, dtype=F32)
        b[:len(v)] = torch.tensor(v, dtype=F64).to(F32)
        assert len(set(b[:len(v)].tolist())) == len(v) == 263
        return b
    return _cached("far", make)


def nonfinite_bias():
    """(512,) fp32: NaN, +inf, -inf in columns 0, 1, 2 and again in the last three (another tile, another wave), the far values between."""
    b = far_values().clone()
    b[:3] = torch.tensor(NONFINITE)
    b[-3:] = torch.tensor(NONFINITE)
    return b


def far_case(dt, nonfinite=False):
    """(c): (256, 512, 256), A = 0 -> pre[m, n] = bias[n]."""
    def make():
        b = nonfinite_bias() if nonfinite else far_values()
        return dict(a=torch.zeros(FAR_M, FAR_K, dtype=dt), w=torch.ones(FAR_N, FAR_K, dtype=dt), bias=b, alpha=1.0, pre=b.to(F64)[None, :].expand(FAR_M, FAR_N).contiguous())
    return _cached(("far", dt, nonfinite), make)


def scaled_f16_case():
    """fp16 operands reach large pre-activations through the accumulator too: every fp16 value times alpha = 2^16 (to 4.3e9)."""
    m = every_case(F16)
    return dict(m, alpha=F16_ALPHA, pre=m["pre"] * F16_ALPHA)


def fwd_cases(dt):
    """name -> case (all finite) of the forward activations for operand dtype dt."""
    cs = {"every": every_case(dt, BF16 if dt == F32 else dt), "grid": grid_case(dt), "far": far_case(dt)}
    if dt == F32:
        cs["every_f16"] = every_case(F32, F16)
    if dt == F16:
        cs["scaled"] = scaled_f16_case()
    return cs


def saved_values(dt):
    """The saved operand of GELU_BWD / u of alpro_gelu_bwd, (rows, 256) of dt: every 16-bit value; for fp32 the grids of (b) and the values of (c)."""
    if dt != F32:
        return every16(dt)
    return _cached("saved32", lambda: torch.cat([grid_points().to(F32), far_values().view(2, 256)]))


def bwd_factor(rows, cols=256):
    """The exact factors of the backward forms, (rows, cols) fp64: row m carries (1, -1, 2)[m % 3] -- GELU_BWD: the row's pre-activation."""
    return torch.tensor([1.0, -1.0, 2.0], dtype=F64)[torch.arange(rows) % 3][:, None].expand(rows, cols).contiguous()
