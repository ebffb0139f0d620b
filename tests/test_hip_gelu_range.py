"""GPU: the GELU epilogues over every 16-bit input, the fp32 grid between them and the far tails (tests/gelu_cases.py), on every route
that reaches one of the six forms of csrc/common.hpp -- alpro_gemm's 128 x 128 kernel (full tiles and the predicated N = 200 path), the
persistent 256 x 256 kernel and the 8-phase kernel (register epilogue, staged epilogue, tile-layout C2) with ACT_GELU, ACT_GELU_SAVE_GRAD
and ACT_GELU_BWD, alpro_gelu_bwd and alpro_gemm_rows_f32.  The weights only select, so each kernel sees exactly the fp32 pre-activation the
fp64 reference sees, and every output must lie in [rn_D(ref - tol), rn_D(ref + tol)] with tol_y = E |x| + 4 2^-24 |ref| + 2^-126 and
tol_dy = E + 4 2^-24 (1 + |x| phi(x)) + 2^-126: no rtol / atol.  E = 3.4e-7 for the 2^q forms, 3.2e-7 for gelu_and_grad2 (the bounds stated
in common.hpp); for the libm forms (erff / __expf) the worst |Phi error| measured on an MI355X is 1.83 x 2^-24 (printed again by every
run of the fp32 cases), asserted at twice that, 3.66 x 2^-24 = 2.18e-7, and never above 8 x 2^-24.  Finite in, finite out -- before its polynomial
argument was limited, gelu_and_grad2 (the SAVE_GRAD form of the 256-tile routes) gave NaN from |x| ~ 7.4e4 -- and NaN in, NaN out, through
ReLU as well.  Each check prints its worst error / tol.
"""
import pytest
import torch

from tests import gelu_cases as gl
from tests import gemm_cases as gc
from tests.gelu_cases import BF16, F16, F32, F64
from tests.test_hip_gemm_exact import _hip, options

pytestmark = pytest.mark.gpu

ROUTES = {      # name -> (library options, columns of the case that are used)
    "k128": (gc.ROUTE_OPTS["k128"], None),
    "k128_n200": (gc.ROUTE_OPTS["k128"], 200),                       # the predicated scalar path
    "p256": (gc.ROUTE_OPTS["p256"], None),
    "q8": (gc.ROUTE_OPTS["q8"], None),                               # register epilogue (pair forms)
    "q8_staged": (gc.ROUTE_OPTS["q8"] + (("gemm_epi", 0),), None),    # the 8-phase kernel's staged 16-bit epilogue
}
DT_ID = {F32: "f32", BF16: "bf16", F16: "f16"}


def form_E(route, dt, out, act):
    """The Phi bound of the form the route runs: the pair form gelu_and_grad2 where a 256-tile route stores 16-bit gelu and gelu' together
    (epi_rows16_c16 of csrc/gemm_epilogue.hpp, the register epilogue of gemm_nt256q_kernels.hpp), the scalar 2^q forms elsewhere."""
    if dt == F32:
        return gl.E_LIBM
    pair = act == gc.ACT_GELU_SAVE_GRAD and out != F32 and route in ("p256", "q8", "q8_staged", "q8_tiled")
    return gl.E_PAIR if pair else gl.E_2Q


def _fwd_params():
    ps = []
    for route in ROUTES:
        for dt in (F32, BF16, F16):
            if dt == F32 and route.startswith("q8"):
                continue
            for out in ((F32,) if dt == F32 else (dt,) if route.startswith("q8") else (dt, F32)):      # (the 8-phase kernel has no fp32-output activation)
                for act in (gc.ACT_GELU, gc.ACT_GELU_SAVE_GRAD):
                    ps.append(pytest.param(route, dt, out, act, id="%s-%s-o%s-%s" % (route, DT_ID[dt], "32" if out == F32 else "16", "gelu" if act == gc.ACT_GELU else "save")))
    return ps


_REFS, _DEV = {}, {}


def refs(c):
    """fp64 references of a case, computed once and shared."""
    k = id(c["pre"])
    if k not in _REFS:
        _REFS[k] = (c["pre"], gl.gelu64(c["pre"]), gl.gelu_grad64(c["pre"]))
    return _REFS[k][1:]


def dev(t):
    k = id(t)
    if k not in _DEV:
        _DEV[k] = (t, t.cuda())
    return _DEV[k][1]


def run_fwd(hip, c, ncols, out, act, pre_act=None, c2_tiled=False):
    a, w = dev(c["a"]), dev(c["w"])
    bias = dev(c["bias"]) if c["bias"] is not None else None
    if ncols:
        w = w[:ncols]
        bias = bias[:ncols] if bias is not None else None
    M, N = a.shape[0], w.shape[0]
    o = torch.full((M, N), float("nan"), dtype=out, device="cuda")
    dy = None
    if act == gc.ACT_GELU_SAVE_GRAD:
        dy = pre_act if pre_act is not None else torch.full((M, N), float("nan"), dtype=a.dtype, device="cuda")
    hip.gemm(a, w, out=o, bias=bias, act=act, out_dtype=out, alpha=c["alpha"], pre_act=dy, c2_tiled=c2_tiled)
    return o, dy


def check(what, got, x, ref, tol, dt, factor=None):
    """Finite in -> finite out (wherever the rounded reference is finite), every element inside its interval; prints the margin."""
    got = got.detach().cpu()
    assert got.dtype == dt and got.shape == x.shape
    fin = gl.must_be_finite(x, ref if factor is None else ref * factor, dt)
    bad_fin = fin & ~got.isfinite()
    assert not bool(bad_fin.any()), "%s: %d finite inputs gave a non-finite output, first x = %r -> %r" % (what, int(bad_fin.sum()), float(x[bad_fin][0]), float(got[bad_fin][0]))
    bad = gl.outside(got, x, ref, tol, dt, factor) & x.isfinite()
    sel = x.isfinite() & got.isfinite()
    if dt == F32:
        margin = "worst error / tol %6.3f" % gl.worst_ratio(got[sel], ref[sel], tol[sel], None if factor is None else factor[sel])
    else:      # a 16-bit output adds its rounding to the error: the margin is the smallest of a few fractions of tol whose interval still holds all
        s = next((s for s in (0.0, 0.25, 0.5, 0.75) if not bool((gl.outside(got, x, ref, s * tol, dt, factor) & x.isfinite()).any())), 1.0)
        margin = "inside at %4.2f x tol      " % s
    moved = int((got.to(F64)[sel] != (ref if factor is None else ref * factor).to(dt).to(F64)[sel]).sum())
    print("%-64s %s   %6d of %6d differ from the rounded reference   outside %d" % (what, margin, moved, int(sel.sum()), int(bad.sum())))
    assert not bool(bad.any()), "%s: %d outside the interval, first x = %r: got %r, reference %r +- %.3e" % (
        what, int(bad.sum()), float(x[bad][0]), float(got[bad][0]), float(ref[bad][0]), float(tol[bad][0]))


def check_fwd(what, c, ncols, o, dy, E, out, dt):
    x = c["pre"][:, :ncols] if ncols else c["pre"]
    ry, rd = (r[:, :ncols] if ncols else r for r in refs(c))
    check(what + " y", o, x, ry, gl.tol_y(x, E), out)
    if dy is not None:
        check(what + " dy", dy, x, rd, gl.tol_dy(x, E), dt)


def check_nonfinite(what, x, y, dy):
    """NaN -> NaN (y and gelu'); +inf -> a non-finite y (torch gives NaN in fp32: both accepted); -inf -> -0, 0 or NaN."""
    y = y.detach().cpu().to(F64)
    nan, pinf, ninf = x.isnan(), x == float("inf"), x == float("-inf")
    assert int(nan.sum()) and int(pinf.sum()) and int(ninf.sum())
    assert bool(y[nan].isnan().all()), "%s: NaN in, %r out" % (what, y[nan][:4].tolist())
    assert not bool(y[pinf].isfinite().any()), "%s: +inf in, %r out" % (what, y[pinf][:4].tolist())
    assert bool((y[ninf].isnan() | (y[ninf] == 0)).all()), "%s: -inf in, %r out" % (what, y[ninf][:4].tolist())
    if dy is not None:
        assert bool(dy.detach().cpu()[nan].isnan().all()), "%s: NaN in, gelu' %r" % (what, dy.detach().cpu()[nan][:4].tolist())


def phi_error_u24(y, x, ry):
    """Worst |Phi error| seen through y / x of an fp32 output, in units of 2^-24 (the libm forms' E is measured with this)."""
    sel = x.isfinite() & (x.abs() >= 2.0 ** -20) & (x.abs() <= 2.0 ** 20)
    return float(((y.detach().cpu().to(F64)[sel] - ry[sel]) / x[sel]).abs().max()) / gl.U24


@pytest.mark.parametrize("route,dt,out,act", _fwd_params())
def test_gelu_forward_range(route, dt, out, act):
    hip = _hip()
    opts, ncols = ROUTES[route]
    E = form_E(route, dt, out, act)
    with options(hip, opts):
        for name, c in gl.fwd_cases(dt).items():
            M, K = c["a"].shape
            if route.startswith("q8"):
                assert hip.gemm_c2_tiled_rows(M, c["w"].shape[0], K, dt) > 0, "%s %s: not routed to the 8-phase kernel" % (route, name)
            o, dy = run_fwd(hip, c, ncols, out, act)
            what = "%s %s o%s %s %s" % (route, DT_ID[dt], DT_ID[out], "gelu" if act == gc.ACT_GELU else "save", name)
            check_fwd(what, c, ncols, o, dy, E, out, dt)
            if dt == F32:
                x = c["pre"][:, :ncols] if ncols else c["pre"]
                print("%-64s libm |Phi error| through y / x: %.2f x 2^-24" % (what, phi_error_u24(o, x, refs(c)[0][:, :ncols] if ncols else refs(c)[0])))
        c = gl.far_case(dt, nonfinite=True)
        o, dy = run_fwd(hip, c, ncols, out, act)
        x = c["pre"][:, :ncols] if ncols else c["pre"]
        check_nonfinite("%s %s non-finite" % (route, DT_ID[dt]), x, o, dy)
        check_fwd("%s %s o%s finite columns of the non-finite launch" % (route, DT_ID[dt], DT_ID[out]), c, ncols, o, dy, E, out, dt)


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_gelu_save_grad_tile_layout(dt):
    """8-phase kernel, c2_tiled: gelu' goes to the tile layout and is read back by MUL_SAVED with pre-activations of exactly 1 -- the 16-bit
    product is then the saved gelu' bit for bit, in row order."""
    hip = _hip()
    with options(hip, gc.ROUTE_OPTS["q8"]):
        for name, c in gl.fwd_cases(dt).items():
            (M, K), N = c["a"].shape, c["w"].shape[0]
            rows = hip.gemm_c2_tiled_rows(M, N, K, dt)
            assert rows == M
            u_tile = torch.full((rows, N), float("nan"), dtype=dt, device="cuda")
            o, _ = run_fwd(hip, c, None, dt, gc.ACT_GELU_SAVE_GRAD, pre_act=u_tile, c2_tiled=True)
            one_a, one_w = torch.zeros(M, K, dtype=dt, device="cuda"), torch.zeros(N, K, dtype=dt, device="cuda")
            one_a[:, 0] = 1
            one_w[:, 0] = 1
            dy = hip.gemm(one_a, one_w, act=gc.ACT_MUL_SAVED, pre_act=u_tile, c2_tiled=True)
            check_fwd("q8_tiled %s %s" % (DT_ID[dt], name), c, None, o, dy, form_E("q8_tiled", dt, dt, gc.ACT_GELU_SAVE_GRAD), dt, dt)
            o2, dy2 = run_fwd(hip, c, None, dt, gc.ACT_GELU_SAVE_GRAD)
            assert torch.equal(o.view(torch.int16), o2.view(torch.int16)) and torch.equal(dy.view(torch.int16), dy2.view(torch.int16)), "tile layout and row layout differ (%s)" % name


def _bwd_params():
    return [pytest.param(r, dt, out, id="%s-%s-o%s" % (r, DT_ID[dt], "32" if out == F32 else "16")) for r in ("k128", "p256") for dt in (F32, BF16, F16)
            for out in ((F32,) if dt == F32 else (dt, F32))]


@pytest.mark.parametrize("route,dt,out", _bwd_params())
def test_gelu_bwd_epilogue_range(route, dt, out):
    """ACT_GELU_BWD: out = pre * gelu'(saved) with pre exactly 1, -1 or 2 per row."""
    hip = _hip()
    saved = gl.saved_values(dt)
    R, K = saved.shape[0], 128
    f = gl.bwd_factor(R)
    a, w = torch.zeros(R, K, dtype=dt), torch.zeros(256, K, dtype=dt)
    a[:, 0] = f[:, 0].to(dt)
    w[:, 0] = 1
    with options(hip, gc.ROUTE_OPTS[route]):
        o = hip.gemm(a.cuda(), w.cuda(), act=gc.ACT_GELU_BWD, out_dtype=out, pre_act=dev(saved))
    x = saved.to(F64)
    E = gl.E_LIBM if dt == F32 else gl.E_2Q
    check("%s %s o%s gelu_bwd epilogue" % (route, DT_ID[dt], DT_ID[out]), o, x, gl.gelu_grad64(x), gl.tol_dy(x, E), out, factor=f)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_gelu_bwd_kernel_range(dt):
    """alpro_gelu_bwd (erff / __expf for every dtype): du = dh * gelu'(u), dh in {1, -2}; 24 elements beyond whole rows, so the element count
    is no multiple of the grid stride (nor of a workgroup's 256 chunks)."""
    hip = _hip()
    u = gl.saved_values(dt).flatten()
    u = torch.cat([u, u[1000:1024]])
    f = torch.where(torch.arange(u.numel()) % 3 == 0, -2.0, 1.0).to(F64)
    du = hip.gelu_bwd(f.to(dt).cuda(), u.cuda())
    x = u.to(F64)
    ref = gl.gelu_grad64(x)
    check("gelu_bwd %s" % DT_ID[dt], du, x, ref, gl.tol_dy(x, gl.E_LIBM), dt, factor=f)
    if dt == F32:
        print("gelu_bwd f32: worst |gelu' error| %.2f x 2^-24" % (float((du.cpu().to(F64) / f - ref)[x.isfinite()].abs().max()) / gl.U24))


@pytest.mark.parametrize("K", [768, 64], ids=["k768_8waves", "k64_4waves"])
def test_gemm_rows_gelu_range(K):
    """alpro_gemm_rows_f32 (gelu_erf): grids (b) and the far values of (c), selected by an identity block of W."""
    hip = _hip()
    x32 = gl.saved_values(F32)
    N = min(K, 256)
    x32 = x32.reshape(-1, N)
    a = torch.zeros(x32.shape[0], K, dtype=F32)
    a[:, :N] = x32
    y = hip.gemm_rows(a.cuda(), torch.eye(N, K, dtype=F32).cuda(), act=gc.ACT_GELU)
    x = x32.to(F64)
    ry = gl.gelu64(x)
    check("gemm_rows K = %d" % K, y, x, ry, gl.tol_y(x, gl.E_LIBM), F32)
    print("gemm_rows K = %d: libm |Phi error| through y / x: %.2f x 2^-24" % (K, phi_error_u24(y, x, ry)))
    b = gl.nonfinite_bias()[:N].clone()
    yb = hip.gemm_rows(torch.zeros(64, K, dtype=F32).cuda(), torch.eye(N, K, dtype=F32).cuda(), bias=b.cuda(), act=gc.ACT_GELU)
    check_nonfinite("gemm_rows K = %d" % K, b.to(F64)[None, :].expand(64, N), yb, None)


def _relu_params():
    return [pytest.param(r, dt, out, id="%s-%s-o%s" % (r, DT_ID[dt], "32" if out == F32 else "16")) for r in ROUTES for dt in (F32, BF16, F16)
            if not (dt == F32 and r.startswith("q8")) for out in ((F32,) if dt == F32 else (dt,) if r.startswith("q8") else (dt, F32))]


@pytest.mark.parametrize("route,dt,out", _relu_params())
def test_relu_passes_nan(route, dt, out):
    """ACT_RELU of alpha * acc + bias: NaN stays NaN (as torch.relu and alpro_gemm_rows_f32; fmaxf hid it as 0), +inf stays, -inf gives 0, and
    every finite column keeps its bits."""
    hip = _hip()
    opts, ncols = ROUTES[route]
    c = gl.far_case(dt, nonfinite=True)
    with options(hip, opts):
        o, _ = run_fwd(hip, c, ncols, out, gc.ACT_RELU)
    x = c["pre"][:, :ncols] if ncols else c["pre"]
    want, got = torch.relu(x).to(out), o.cpu()
    assert bool(got[x.isnan()].isnan().all()) and int(x.isnan().sum()) >= 256, "%s: NaN pre-activation -> %r" % (route, got[x.isnan()][:4].tolist())
    assert torch.equal(got.isnan(), want.isnan()) and torch.equal(torch.nan_to_num(got.float(), nan=0.0), torch.nan_to_num(want.float(), nan=0.0))
