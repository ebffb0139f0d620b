"""CPU self-check of tests/gelu_cases.py: the pre-activations are exact in fp32 in every summation order, each case exercises what it claims,
an fp32 restatement of each of the six forms of csrc/common.hpp (coefficients restated here as data, not read from the C++) meets the
interval condition on every case -- except gelu_and_grad2 as it stood before its polynomial argument was limited, which must fail
finite-in / finite-out at +-1e5 -- and the condition rejects four planted faults of the reference.

Which output dtype sees which fault (asserted below, over the (a) + (b) points):
    fault                                   fp32 output   bf16 output   fp16 output
    tanh-form GELU                          rejected      rejected      rejected
    x rounded to the operand dtype first    rejected      rejected      rejected      (grid (b); the operand dtype = the output dtype)
    gelu' without x phi(x)                  rejected      rejected      rejected
    y rounded twice (fp16, then bf16)       --            rejected      --            (a fault of the bf16 store only)
No fault is visible to the fp32-output cases alone; tests/test_hip_gelu_range.py still runs an fp32-output case on every route that has one.
"""
import pytest
import torch

from tests import gelu_cases as gl
from tests.gelu_cases import BF16, F16, F32, F64, E_2Q, E_LIBM, E_PAIR, INV_SQRT_2PI, SQRT1_2      # noqa: F401

# ------------------------------------------------------------------------------------------------ fp32 restatements of the six forms
# The coefficients are restated here as data (not read from the C++) and held against the intervals of tests/gelu_cases.py below.
# Plain fp32 arithmetic without fused multiply-adds: the device may be slightly better, not worse by more than the rounding terms allow.
Q_COEF = (-0.00296695, 0.02966973, -0.14875628, -0.91847146, -1.62789348, -1.0)      # alone: 3.41e-7 on Phi at z = 2.47 even in exact arithmetic
# the constant term rises from -1 to -1 + 2^-12 over z in [2.3, 2.425] and stays there: med3(z * slope + offset, -1, top)
Q_TAIL_SLOPE, Q_TAIL_START, Q_TAIL_TOP = 2.0 ** -9, 2.3, -1.0 + 2.0 ** -12
P_COEF = (-8.062383613e-06, 1.519315725e-04, -1.271098853e-03, 6.382599637e-03, -2.223049180e-02, 5.949637600e-02, -1.317726293e-01,
          2.497522130e-01, -3.989226083e-01, 4.999997430e-01)
LOG2E_HALF_NEG = -0.72134752044448170368
PAIR_T_MAX = 13.0          # gelu_and_grad2 evaluates its polynomial at min(|x|, 13): the fit's range; beyond it exp(-x^2 / 2) * g is below 2^-121


def _f(c):
    return torch.tensor(c, dtype=F32)


def _horner(coef, t):
    p = t * _f(coef[0]) + _f(coef[1])
    for c in coef[2:]:
        p = p * t + _f(c)
    return p


def r_half_erfc_pos(z, tail=True):
    """tail=False: the polynomial alone, as the form stood before the constant term was raised in the tail."""
    z = z.to(F32)
    if not tail:
        return torch.exp2(_horner(Q_COEF, z))
    offset = _f(-1.0) - _f(Q_TAIL_START) * _f(Q_TAIL_SLOPE)
    c = torch.minimum(torch.maximum(z * _f(Q_TAIL_SLOPE) + offset, _f(-1.0)), _f(Q_TAIL_TOP))
    return torch.exp2(_horner(Q_COEF[:-1], z) * z + c)


def _cdf_from_h(h, x):
    return _f(0.5) + torch.copysign(_f(0.5) - h, x)


def r_gelu_fast(x):
    x = x.to(F32)
    return x * _cdf_from_h(r_half_erfc_pos(x.abs() * _f(SQRT1_2)), x)


def r_gelu_grad(x):
    x = x.to(F32)
    pdf = _f(INV_SQRT_2PI) * torch.exp2(x * x * _f(LOG2E_HALF_NEG))
    return _cdf_from_h(r_half_erfc_pos(x.abs() * _f(SQRT1_2)), x) + x * pdf


def r_gelu_and_grad(x):
    return r_gelu_fast(x), r_gelu_grad(x)


r_gelu_fast2 = r_gelu_fast      # the same arithmetic on 2-vectors


def r_gelu_and_grad2(x, clamp=True):
    """clamp=False: the form as it stood before the polynomial's argument was limited (p overflows to -inf from |x| ~ 7.4e4 while e is 0)."""
    x = x.to(F32)
    t = x.abs().clamp(max=PAIR_T_MAX) if clamp else x.abs()
    p = _horner(P_COEF, t)
    e = torch.exp2(x * x * _f(LOG2E_HALF_NEG))
    cdf = _cdf_from_h(e * p, x)
    return x * cdf, cdf + x * (e * _f(INV_SQRT_2PI))


def r_gelu_erf(x):
    x = x.to(F32)
    return _f(0.5) * x * (_f(1.0) + torch.erf(x * _f(SQRT1_2)))


def r_gelu_and_grad_libm(x):
    x = x.to(F32)
    cdf = _f(0.5) * (_f(1.0) + torch.erf(x * _f(SQRT1_2)))
    return x * cdf, cdf + x * _f(INV_SQRT_2PI) * torch.exp(_f(-0.5) * x * x)


# ------------------------------------------------------------------------------------------------ the cases
DTS = [F32, BF16, F16]
DT_IDS = ["f32", "bf16", "f16"]


def all_finite_points():
    """Every pre-activation of (a) (both 16-bit dtypes and fp16 times 2^16), (b) and the finite part of (c), as one fp64 vector."""
    return gl._cached("cpu_points", lambda: torch.cat([gl.every16(BF16).to(F64).flatten(), gl.every16(F16).to(F64).flatten(), gl.scaled_f16_case()["pre"].flatten(),
                                                       gl.grid_points().flatten(), gl.far_values().to(F64)]))


def test_every16_holds_65536_distinct_patterns():
    for dt, nonfinite in ((BF16, 2 * 128), (F16, 2 * 1024)):
        raw = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt)
        assert raw.view(torch.int16).unique().numel() == 65536 and int((~raw.isfinite()).sum()) == nonfinite
        ev = gl.every16(dt)
        assert ev.shape == (256, 256) and bool(ev.isfinite().all())
        keep = raw.isfinite()
        assert torch.equal(ev.flatten()[keep].view(torch.int16), raw[keep].view(torch.int16))      # every finite pattern, bit for bit (-0 and subnormals included)
        assert bool((ev.flatten()[~keep].view(torch.int16) == 0).all())
        assert ev.view(torch.int16).unique().numel() == 65536 - nonfinite
        tiny = torch.finfo(dt).tiny
        assert bool(((ev.float().abs() < tiny) & (ev != 0)).any()) and float(ev.float().abs().max()) == torch.finfo(dt).max


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_grid_pieces_add_up_exactly_in_fp32(dt):
    gp = gl.grid_points()
    assert gp.shape == (gl.GRID_ROWS, 256) and gp.numel() == 65536 + 2 * 2 ** 14 and gp.unique().numel() == gp.numel() - 1      # (-8 ends one grid and starts the other)
    assert float(gp.min()) == -16.0 + 2.0 ** -11 and float(gp.max()) == 16.0 - 2.0 ** -11 and bool((gp[:256].flatten().diff() == 2.0 ** -12).all())
    hi, lo = gl.split_hi_lo(gp, dt)
    assert hi.dtype == lo.dtype == dt
    assert torch.equal((hi.to(F32) + lo.to(F32)).to(F64), gp) and torch.equal((lo.to(F32) + hi.to(F32)).to(F64), gp)
    assert torch.equal(gp.to(F32).to(F64), gp)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_pre_activations_are_exact_in_fp32_in_any_summation_order(dt):
    for name, c in gl.fwd_cases(dt).items():
        K = c["a"].shape[1]
        perm = torch.randperm(K, generator=torch.Generator().manual_seed(K + len(name)))
        a, w = c["a"].to(F32)[:, perm].contiguous(), c["w"].to(F32)[:, perm].contiguous()
        pre = c["alpha"] * (a @ w.T) + (c["bias"] if c["bias"] is not None else 0.0)
        assert pre.dtype == F32 and torch.equal(pre.to(F64), c["pre"]), name
        assert int((c["w"] != 0).sum(1).max()) <= (2 if name != "far" else K) and bool(c["pre"].isfinite().all())
    nf = gl.far_case(dt, nonfinite=True)
    assert nf["pre"][0, :3].isnan().tolist() == [True, False, False] and nf["pre"][0, 1] == float("inf") and nf["pre"][0, -1] == float("-inf")


def test_far_values_are_the_listed_ones():
    b = gl.far_values().to(F64)
    for v in [2.0 ** 4, -2.0 ** 127, 7e4, -7.5e4, 1e5, -1e5, 1e10, 3e38, -3e38, 2.0 ** -126, 2.0 ** -140]:
        assert bool((b == float(torch.tensor(v, dtype=F32))).any()), v


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_grid_outputs_exercise_the_16_bit_rounding(dt):
    """At least 5 % of the grid's fp32 results are not representable in the 16-bit output type (judged from the reference alone)."""
    x = gl.grid_points()
    for ref in (gl.gelu64(x), gl.gelu_grad64(x)):
        r32 = ref.to(F32)
        assert float((r32.to(dt).to(F32) != r32).double().mean()) >= 0.05


def test_reference_keeps_the_negative_tail():
    """Against libm's erfc (math.erfc), an implementation independent of torch's: relative agreement down to gelu(-30) = -1.5e-196, where
    1 + erf has long been 0."""
    import math
    xs = [-0.5, -3.0, -6.0, -10.0, -20.0, -30.0]
    x = torch.tensor(xs, dtype=F64)
    want = torch.tensor([v * 0.5 * math.erfc(-v / math.sqrt(2.0)) for v in xs], dtype=F64)
    assert bool((want < 0).all()) and torch.allclose(gl.gelu64(x), want, rtol=1e-12, atol=0.0)
    want_d = torch.tensor([0.5 * math.erfc(-v / math.sqrt(2.0)) + v * math.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi) for v in xs], dtype=F64)
    assert torch.allclose(gl.gelu_grad64(x), want_d, rtol=1e-9, atol=0.0)
    assert float(gl.gelu64(torch.tensor(-0.0, dtype=F64))) == 0.0 and float(gl.gelu64(torch.tensor(-3e38, dtype=F64))) == 0.0


# ------------------------------------------------------------------------------------------------ the restatements meet the condition
FORMS = {      # name -> (x -> (y or None, dy or None), E)
    "gelu_erf": (lambda x: (r_gelu_erf(x), None), E_LIBM),
    "gelu_and_grad_f32": (r_gelu_and_grad_libm, E_LIBM),
    "gelu_fast": (lambda x: (r_gelu_fast(x), None), E_2Q),
    "gelu_grad": (lambda x: (None, r_gelu_grad(x)), E_2Q),
    "gelu_and_grad": (r_gelu_and_grad, E_2Q),
    "gelu_fast2": (lambda x: (r_gelu_fast2(x), None), E_2Q),
    "gelu_and_grad2": (r_gelu_and_grad2, E_PAIR),
}


@pytest.mark.parametrize("name", list(FORMS))
def test_restatement_meets_the_interval_on_every_case(name):
    fn, E = FORMS[name]
    x = all_finite_points()
    y, dy = fn(x)
    for what, got, ref, tol in (("y", y, gl.gelu64(x), gl.tol_y(x, E)), ("dy", dy, gl.gelu_grad64(x), gl.tol_dy(x, E))):
        if got is None:
            continue
        assert got.dtype == F32 and bool(got.isfinite().all()), "%s %s: a finite input gave a non-finite output" % (name, what)
        bad = gl.outside(got, x, ref, tol, F32)
        print("%s %s: worst error / tol %.3f over %d points" % (name, what, gl.worst_ratio(got, ref, tol), x.numel()))
        assert not bool(bad.any()), "%s %s: %d outside, first at x = %r" % (name, what, int(bad.sum()), float(x[bad][0]))
        for dt in (BF16, F16):      # rounding is monotonic: the rounded result is inside the rounded interval
            assert not bool(gl.outside(got.to(dt), x, ref, tol, dt).any())


def test_half_erfc_pos_meets_its_phi_bound():
    """The form in exact arithmetic (the fp32 constants in fp64) is within 3.1e-7 of 0.5 erfc -- E_2Q less the 2^-26 that 0.5 - (0.5 - h) can
    lose for a negative x and a margin -- and its fp32 evaluation within E_2Q plus 4 ulp of the value (the allowance tol_y makes); the
    polynomial alone misses E_2Q at z = 2.47 even in exact arithmetic; the tail term changes no bit below z = 2.29, never raises 2^q above
    erfc, and never gives a NaN."""
    z = torch.linspace(0.0, 12.0, 1_200_001, dtype=F64)
    want = 0.5 * torch.special.erfc(z)

    def exact(tail):
        q = z * float(_f(Q_COEF[0])) + float(_f(Q_COEF[1]))
        for c in Q_COEF[2:-1]:
            q = q * z + float(_f(c))
        c = ((z - Q_TAIL_START) * Q_TAIL_SLOPE - 1.0).clamp(-1.0, Q_TAIL_TOP) if tail else -1.0
        return torch.exp2(q * z + c)
    fit, alone = exact(True) - want, (exact(False) - want).abs()
    err32 = (r_half_erfc_pos(z).to(F64) - want).abs()
    print("half_erfc_pos: exact arithmetic %.3e, fp32 evaluation %.3e (bound %.1e); the polynomial alone %.4e at z = %.2f"
          % (float(fit.abs().max()), float(err32.max()), E_2Q, float(alone.max()), float(z[alone.argmax()])))
    assert float(fit.abs().max()) <= 3.1e-7 and bool((err32 <= E_2Q + 4.0 * gl.U24 * want).all())
    assert float(alone.max()) > E_2Q and 2.4 < float(z[alone.argmax()]) < 2.55
    assert bool((fit[z > Q_TAIL_START] < 0).all())
    below = z[z <= 2.29]
    assert torch.equal(r_half_erfc_pos(below), r_half_erfc_pos(below, tail=False)) and not torch.equal(r_half_erfc_pos(z), r_half_erfc_pos(z, tail=False))
    big = torch.tensor([1e3, 1e5, 1e20, 2.4e38, float("inf")])
    assert r_half_erfc_pos(big).tolist() == [0.0] * 5 and bool(r_half_erfc_pos(torch.tensor([float("nan")])).isnan().all())


def test_pair_form_without_the_limit_fails_finite_out_at_1e5():
    """The defect the range tests were written against, pinned on the CPU: before its polynomial argument was limited to the fit's range,
    gelu_and_grad2 returned NaN for y and dy from |x| ~ 7.4e4 (0 * -inf); the limited form is finite and inside the interval."""
    x = torch.tensor([7e4, -7e4, 1e5, -1e5, 1e6, 1e10, 3e38, -3e38], dtype=F64)
    y0, d0 = r_gelu_and_grad2(x, clamp=False)
    assert y0.isnan().tolist() == d0.isnan().tolist() == [False, False, True, True, True, True, True, True]
    assert bool(gl.outside(y0, x, gl.gelu64(x), gl.tol_y(x, E_PAIR), F32)[2:].all())
    y1, d1 = r_gelu_and_grad2(x)
    assert bool(y1.isfinite().all()) and bool(d1.isfinite().all())
    assert not bool(gl.outside(y1, x, gl.gelu64(x), gl.tol_y(x, E_PAIR), F32).any()) and not bool(gl.outside(d1, x, gl.gelu_grad64(x), gl.tol_dy(x, E_PAIR), F32).any())
    near = torch.linspace(-13.5, 13.5, 540_001, dtype=F64)      # the limit changes nothing the bound could see on either side of 13
    a, b = r_gelu_and_grad2(near), r_gelu_and_grad2(near, clamp=False)
    assert torch.equal(a[0], b[0]) and float((a[1] - b[1]).abs().max()) <= 2.0 ** -126


def test_nonfinite_inputs_of_the_restatements():
    x = torch.tensor(gl.NONFINITE, dtype=F64)
    for name, (fn, _) in FORMS.items():
        for got in fn(x):
            if got is not None:
                assert bool(got[0].isnan()), name


# ------------------------------------------------------------------------------------------------ the condition rejects planted faults
def _rejects(got64, x, ref, tol, dt):
    return bool(gl.outside(got64.to(dt), x, ref, tol, dt).any())


def test_interval_rejects_planted_faults():
    """See the table in the module docstring: every row of it is asserted here, with the tighter of the two 16-bit-form bounds' tolerances
    replaced by the WIDER one (E_2Q), so that a rejection holds under every E the GPU test uses for 16-bit operands."""
    E = max(E_2Q, E_LIBM, E_PAIR)
    xa = torch.cat([gl.every16(BF16).to(F64).flatten(), gl.every16(F16).to(F64).flatten(), gl.grid_points().flatten()])
    ref_y, t_y, ref_d, t_d = gl.gelu64(xa), gl.tol_y(xa, E), gl.gelu_grad64(xa), gl.tol_dy(xa, E)
    for dt in (F32, BF16, F16):
        assert not _rejects(ref_y, xa, ref_y, t_y, dt) and not _rejects(ref_d, xa, ref_d, t_d, dt)      # the reference itself passes
        assert _rejects(gl.gelu64(xa, fault="tanh"), xa, ref_y, t_y, dt), "tanh form, %s output" % dt
        assert _rejects(gl.gelu_grad64(xa, fault="no_x_phi"), xa, ref_d, t_d, dt), "gelu' without x phi(x), %s output" % dt
    xg = gl.grid_points().flatten()
    ref_g, t_g = gl.gelu64(xg), gl.tol_y(xg, E)
    for op_dt in (BF16, F16):
        early = gl.gelu64(xg.to(op_dt).to(F64))
        for dt in (F32, op_dt):
            assert _rejects(early, xg, ref_g, t_g, dt), "x rounded to %s before the GELU, %s output" % (op_dt, dt)
    twice = ref_y.to(F16).to(F64)
    inside_f16 = ref_y.abs() < 60000.0
    assert bool(gl.outside(twice.to(BF16), xa, ref_y, t_y, BF16)[inside_f16].any()), "y rounded through fp16 and then bf16"
    assert not _rejects(ref_y.to(BF16).to(F64), xa, ref_y, t_y, BF16)


def test_backward_factor_scales_the_interval():
    x = gl.saved_values(F32).to(F64)
    f = gl.bwd_factor(x.shape[0])
    assert sorted(f[:, 0].unique().tolist()) == [-1.0, 1.0, 2.0]
    ref, tol = gl.gelu_grad64(x), gl.tol_dy(x, E_LIBM)
    good = (r_gelu_and_grad_libm(x)[1].to(F64) * f).to(F32)
    assert not bool(gl.outside(good, x, ref, tol, F32, factor=f).any())
    assert bool(gl.outside(-good, x, ref, tol, F32, factor=f).any()) and bool(gl.outside(good, x, ref, tol, F32).any())
