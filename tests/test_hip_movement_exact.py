"""GPU: the kernels that only move rows (tests/movement_cases.py) bit for bit -- transposes, the index-mapped gather, the scatters, the
fusion-sequence gather and its backward, patchify, the CLS-mean backward -- on inputs whose result is exact in every summation order, with
ZERO tolerance, inside poisoned surroundings: sources in NaN-filled buffers, outputs and destination tables in sentinel-filled ones whose
guard rows and columns must keep their bits.  The three kernels that promise a summation order run a second time on fp32 data with a wide
exponent spread against the CPU emulation of exactly that order, and twice for run-to-run equality.  alpro_gelu_bwd, the one inexact kernel
of the group, keeps the tolerances of tests/test_hip_bwd_ops.py and adds its exact properties.

Every index handed to a kernel that does not range-check is in range; out-of-range indices go only to the ordered scatter, which documents
them as dropped."""
import pytest
import torch

from tests import movement_cases as mc
from tests.gemm_cases import DT_NAME, F32, MAP_FRAME_TOKENS, MAP_IDENTITY, MAP_PATCH_EMBED, MAP_SKIP_CLS, SENTINEL, gen, ints, poisoned, poisoned_vec
from tests.test_hip_bwd_ops import _determinism
from tests.test_hip_ops import close

pytestmark = pytest.mark.gpu
D, G = mc.D, mc.GUARD


def _hip():
    from alpro_amd import hip
    hip.load()
    assert (hip.MAP_IDENTITY, hip.MAP_SKIP_CLS, hip.MAP_FRAME_TOKENS, hip.MAP_PATCH_EMBED) == (MAP_IDENTITY, MAP_SKIP_CLS, MAP_FRAME_TOKENS, MAP_PATCH_EMBED)
    return hip


def sentinel_view(rows, cols, dt, guard_cols=0):
    """A (rows, cols) view at row G of a sentinel-filled device buffer with G guard rows on both sides and guard_cols columns behind."""
    buf = torch.full((G + rows + G, cols + guard_cols), SENTINEL, dtype=dt, device="cuda")
    return buf[G:G + rows, :cols]


def assert_same(got, want, what):
    assert mc.same(got, want), "%s: first mismatch (row, column, got, want) %s" % (what, mc.first_mismatch(got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])))


# ------------------------------------------------------------------------------------------------ transpose
def _transpose_into(hip, x, out, R, C, Rpad, colsum):
    """alpro_transpose through the wrapper's own handle and pointer helpers, into a caller-owned (sentinel-surrounded) output."""
    hip._check(hip.load().alpro_transpose(hip._ptr(x), hip.dtype_code(x.dtype), x.stride(0), hip._ptr(out), hip.dtype_code(out.dtype), out.stride(0), R, C, Rpad,
                                          hip._ptr(colsum), hip._stream()), "alpro_transpose")


@pytest.mark.parametrize("pad_to", mc.TR_PADS)
@pytest.mark.parametrize("din,dout", mc.TR_DTYPES, ids=["%s_%s" % (DT_NAME[a], DT_NAME[b]) for a, b in mc.TR_DTYPES])
def test_transpose_exact(din, dout, pad_to):
    hip = _hip()
    for c in (c for c in mc.TRANSPOSE_CASES if (c.din, c.dout, c.pad_to) == (din, dout, pad_to)):
        what = mc.tr_id(c)
        t = mc.transpose_inputs(c)
        Rp = mc.rpad(c.R, pad_to)
        x = poisoned(t["x"].to(din), 3, 8 if c.strided else 0, 1, device="cuda")
        assert x.stride(0) == c.C + (8 if c.strided else 0)
        ref = mc.transpose_ref(t["x"], Rp).to(dout)
        want_cs = poisoned_vec(t["colsum"].to(F32), 8, fill=SENTINEL)._base
        for det in (True, False):      # the wrapper: column sums in the default (fixed-order) mode and fused into the kernel
            with _determinism(hip, det):
                cs = poisoned_vec(t["colsum0"], 8, fill=SENTINEL, device="cuda")
                out = hip.transpose(x, out_dtype=dout, pad_to=pad_to, colsum=cs)
            assert_same(out, ref, "%s det=%s" % (what, det))
            assert_same(cs._base[None], want_cs[None], "%s det=%s colsum" % (what, det))
        out = sentinel_view(c.C, Rp, dout, mc.TR_GUARD_COLS)
        cs = poisoned_vec(t["colsum0"], 8, fill=SENTINEL, device="cuda")
        _transpose_into(hip, x, out, c.R, c.C, Rp, cs)
        assert_same(out._base, mc.transpose_expected(t["x"], Rp, dout), what + " buffer")
        assert mc.pad_is_plus_zero(out._base, c.C, c.R, Rp), what + " pad columns"
        assert_same(cs._base[None], want_cs[None], what + " fused colsum")


@pytest.mark.parametrize("dout", mc.DTS, ids=[DT_NAME[d] for d in mc.DTS])
@pytest.mark.parametrize("table", sorted(mc.TB_TABLES))
def test_transpose_batch_exact(table, dout):
    hip = _hip()
    jobs = mc.TB_TABLES[table]
    xs = [mc.matrix(R, C, F32, dout, table, j) for j, (R, C, _) in enumerate(jobs)]
    srcs = [poisoned(x.to(F32), 2, 8 * (j % 2), 1, device="cuda") for j, x in enumerate(xs)]
    outs = [sentinel_view(C, mc.rpad(R, 64) + extra, dout, 8 + 8 * (j % 3)) for j, (R, C, extra) in enumerate(jobs)]
    assert all(o.stride(0) > o.shape[1] for o in outs)
    tbl, n, tiles = hip.transpose_jobs(list(zip(srcs, outs)))
    assert n == len(jobs) and tiles == sum(((C + 63) // 64) * ((o.shape[1] + 63) // 64) for (R, C, _), o in zip(jobs, outs))
    for _ in range(2):          # the table is built once and launched every step
        hip.transpose_batch(tbl, n, tiles, dout)
    for j, (x, o) in enumerate(zip(xs, outs)):
        R, C, _ = jobs[j]
        what = "%s job %d (%d x %d -> Rpad %d)" % (table, j, R, C, o.shape[1])
        assert_same(o._base, mc.transpose_expected(x, o.shape[1], dout, guard_cols=8 + 8 * (j % 3)), what)
        assert mc.pad_is_plus_zero(o._base, C, R, o.shape[1]), what + " pad columns"


# ------------------------------------------------------------------------------------------------ gather_cast
def _gather_cast_into(hip, src, out, rows, x, c, rs, cs, cp):
    ws, wsb = hip._reduce_ws(src.device) if (cs is not None or cp is not None) else (None, 0)
    hip._check(hip.load().alpro_gather_cast(hip._ptr(src), D, hip._ptr(out), hip.dtype_code(out.dtype), rows, D, c.mode, x.p0, x.p1, hip._ptr(rs), max(c.group, 1), x.cls_scale,
                                            mc.DROP_P if x.drop_seed else 0.0, x.drop_seed, hip._ptr(cs), hip._ptr(cp), ws, wsb, hip._stream()), "alpro_gather_cast")


@pytest.mark.parametrize("c", mc.GATHER_CAST_CASES, ids=[mc.gc_id(c) for c in mc.GATHER_CAST_CASES])
def test_gather_cast_exact(c):
    hip = _hip()
    x = mc.gc_build(c)
    src = poisoned(x.src, 3, 0, 1, device="cuda")
    rs = poisoned_vec(x.row_scale, 8, device="cuda") if x.row_scale is not None else None
    want = mc.gc_expected(c, x)
    want_cs = {k: poisoned_vec(x.ref[k].to(F32), 8, fill=SENTINEL)._base[None] for k in ("colsum", "pre")}

    def sums():
        return (poisoned_vec(x.colsum0, 8, fill=SENTINEL, device="cuda") if c.colsum in ("colsum", "both") else None,
                poisoned_vec(x.pre0, 8, fill=SENTINEL, device="cuda") if c.colsum in ("pre", "both") else None)

    def check_sums(cs, cp, what):
        if cs is not None:
            assert_same(cs._base[None], want_cs["colsum"], what + " colsum")
        if cp is not None:
            assert_same(cp._base[None], want_cs["pre"], what + " colsum_pre")
    with _determinism(hip, c.det):
        cs, cp = sums()
        out = sentinel_view(c.rows, D, c.dt)
        _gather_cast_into(hip, src, out, c.rows, x, c, rs, cs, cp)
        assert_same(out._base, want, mc.gc_id(c))
        check_sums(cs, cp, mc.gc_id(c))
        cs, cp = sums()
        out = hip.gather_cast(src, c.dt, rows=c.rows, map_mode=c.mode, map_p0=x.p0, map_p1=x.p1, row_scale=rs, row_scale_group=max(c.group, 1), cls_scale=x.cls_scale,
                              drop_p=mc.DROP_P if x.drop_seed else 0.0, drop_seed=x.drop_seed, colsum=cs, colsum_pre=cp)
        assert_same(out, want[G:G + c.rows], mc.gc_id(c) + " (wrapper)")
        check_sums(cs, cp, mc.gc_id(c) + " (wrapper)")


# ------------------------------------------------------------------------------------------------ scatters
def _table(V, fill=None):
    """(buffer, table view): V table rows at row G of a buffer whose guard rows hold SENTINEL."""
    buf = torch.full((G + V + G, D), SENTINEL if fill is None else fill, dtype=F32, device="cuda")
    if fill is None:
        buf[G:G + V] = mc.table_fill(torch.arange(V, device="cuda"))
    else:
        buf[:G] = SENTINEL
        buf[G + V:] = SENTINEL
    return buf, buf[G:G + V]


def _expect(buf0, touched, values):
    want = buf0.clone()
    want[G + touched.cuda()] = values.cuda()
    return want


@pytest.mark.parametrize("c", mc.ORDERED_SCATTER_CASES, ids=[mc.sc_id(c) for c in mc.ORDERED_SCATTER_CASES])
def test_scatter_ordered(c):
    hip = _hip()
    x = mc.sc_build(c)
    src, idx = poisoned(x.src, 2, 0, 1, device="cuda"), x.idx.cuda()
    touched, values = mc.sc_expected_rows(x, c.V, c.kind)
    big = c.V == mc.SC_TOP
    buf, dst = _table(c.V, x.fill)
    buf0 = None if big else buf.clone()
    runs = []
    for _ in range(2 if c.kind == "order" else 1):
        # the ordered form is the only one that range-checks: nothing else may see this case's indices
        assert hip.deterministic() and c.rows <= 8192 and dst.shape[0] < (1 << 19) and src.is_contiguous() and dst.is_contiguous()
        hip.scatter_add_rows(src, idx, dst, skip_idx=x.skip)
        if big:     # 1.6 GB: the touched rows, the guards and a strided sample of the rest against the untouched fill
            t = touched.cuda()
            assert set(touched.tolist()) <= {0, c.V - 1}
            assert_same(dst[t], values, mc.sc_id(c) + " touched rows")
            assert bool((buf[:G] == SENTINEL).all()) and bool((buf[G + c.V:] == SENTINEL).all()), "guard rows"
            assert bool((dst[1:c.V - 1:4099] == x.fill).all()) and bool((dst[1:66] == x.fill).all()) and bool((dst[c.V - 66:c.V - 1] == x.fill).all()), "untouched rows"
            runs.append(dst[t].clone())
            dst[t] = x.fill
        else:
            assert_same(buf, _expect(buf0, touched, values), mc.sc_id(c))
            runs.append(buf)
            buf = buf0.clone()
            dst = buf[G:G + c.V]
    assert len(runs) == 1 or torch.equal(runs[0], runs[1]), "two runs differ"


@pytest.mark.parametrize("rows,idx_mod", mc.MOD_CASES)
def test_scatter_position_form(rows, idx_mod):
    hip = _hip()
    kinds = ("exact", "order") if (rows + idx_mod - 1) // idx_mod >= 3 else ("exact",)
    for kind in kinds:
        x = mc.mod_build(rows, idx_mod, kind)
        src = poisoned(x.src, 2, 0, 1, device="cuda")
        touched, values = mc.sc_expected_rows(x, idx_mod, kind)
        want = mc.table_expected(mc.MOD_TABLE_ROWS, touched, values)
        runs = []
        for _ in range(2 if kind == "order" else 1):
            buf, dst = _table(mc.MOD_TABLE_ROWS)
            hip.scatter_add_rows(src, None, dst, idx_mod=idx_mod)
            assert_same(buf, want, "rows %d idx_mod %d %s" % (rows, idx_mod, kind))
            runs.append(buf)
        assert len(runs) == 1 or torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("route", mc.OTHER_ROUTES)
def test_scatter_other_routes(route):
    """The routes that do not range-check -- torch's index_put_ above 8192 rows, the atomic kernel with and without an index vector -- on
    in-range indices and exact inputs against the same fp64 reference."""
    hip = _hip()
    if route in mc.OTHER_ROUTE_CASES:
        det, cases = mc.OTHER_ROUTE_CASES[route]
        for c in cases:
            x = mc.sc_build(c)
            assert bool(((x.idx >= 0) & (x.idx < c.V)).all()), "in-range indices only"
            touched, values = mc.sc_expected_rows(x, c.V, "exact")
            buf, dst = _table(c.V)
            want = _expect(buf, touched, values)
            with _determinism(hip, det):
                hip.scatter_add_rows(poisoned(x.src, 2, 0, 1, device="cuda"), x.idx.cuda(), dst, skip_idx=x.skip)
            assert_same(buf, want, route + " " + mc.sc_id(c))
        return
    for rows, idx_mod, skip in mc.MOD_SKIP_CASES:
        x = mc.mod_skip_build(rows, idx_mod, skip)
        touched, values = mc.sc_expected_rows(x, idx_mod, "exact")
        buf, dst = _table(mc.MOD_TABLE_ROWS)
        with _determinism(hip, mc.MOD_SKIP_ROUTES[route]):
            hip.scatter_add_rows(poisoned(x.src, 2, 0, 1, device="cuda"), None, dst, idx_mod=idx_mod, skip_idx=skip)
        assert_same(buf, mc.table_expected(mc.MOD_TABLE_ROWS, touched, values), "%s rows %d idx_mod %d skip %d" % (route, rows, idx_mod, skip))


# ------------------------------------------------------------------------------------------------ gather_seq
def _pool(t):
    """A pool (P, L, 768) between one NaN pool row before and one behind."""
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), float("nan"), dtype=t.dtype)
    buf[1:-1] = t
    return buf.cuda()[1:-1]


@pytest.mark.parametrize("c", mc.GATHER_SEQ_CASES, ids=[mc.gs_id(c) for c in mc.GATHER_SEQ_CASES])
def test_gather_seq_exact(c):
    hip = _hip()
    x = mc.gs_build(c)
    ti, vi = x.ti.cuda(), x.vi.cuda()
    ref = mc.gs_forward_ref(x)
    out32, out_t = hip.gather_seq(_pool(x.text), _pool(x.video), ti, vi, c.dt)
    assert_same(out32, ref, "out32")
    if c.dt == F32:
        assert out_t is None
    else:
        assert_same(out_t, ref.to(c.dt), "out_t")

    def bwd(kind):
        d_t = x.d_t[kind]
        return hip.gather_seq_bwd(poisoned(x.d32[kind], 2, 0, 1, device="cuda"), None if d_t is None else poisoned(d_t, 2, 0, 1, device="cuda"), ti, vi, c.Pt, c.Pv, c.Lt, c.Lv)
    for got, want, idx, what in zip(bwd("exact"), mc.gs_backward_ref(c, x), (x.ti, x.vi), ("dtext", "dvideo")):
        assert_same(got.view(-1, D), want.view(-1, D), what + " (exact)")
        unused = torch.tensor(sorted(set(range(got.shape[0])) - set(idx.tolist())), dtype=torch.int64)
        assert c.pattern == "identity" or got.shape[0] == 1 or unused.numel() > 0
        assert not bool(got.cpu()[unused].any()), what + ": an unused pool row is not exactly zero"
    a, b = bwd("order"), bwd("order")
    for got, again, want, what in zip(a, b, mc.gs_backward_emulated(c, x), ("dtext", "dvideo")):
        assert_same(got.view(-1, D), want.view(-1, D), what + " (ascending s, d32 before d_t)")
        assert torch.equal(got, again), what + ": two runs differ"


# ------------------------------------------------------------------------------------------------ patchify, cls_mean_bwd, gelu_bwd
@pytest.mark.parametrize("dt", mc.DTS, ids=[DT_NAME[d] for d in mc.DTS])
@pytest.mark.parametrize("shape", mc.PATCHIFY_SHAPES, ids=["x".join(map(str, s)) for s in mc.PATCHIFY_SHAPES])
def test_patchify_exact(shape, dt):
    hip = _hip()
    img = mc.patchify_image(shape, dt)
    ref = mc.patchify_ref(img).to(dt)
    dev = _pool(img)
    BT, C, H, W = shape
    assert_same(hip.patchify(dev, dt), ref, "patchify (wrapper)")
    out = sentinel_view(ref.shape[0], ref.shape[1], dt)
    hip._check(hip.load().alpro_patchify(hip._ptr(dev), hip._ptr(out), hip.dtype_code(dt), BT, C, H, W, hip._stream()), "alpro_patchify")
    assert_same(out._base, poisoned(ref, G, 0, G, fill=SENTINEL)._base, "patchify buffer")


@pytest.mark.parametrize("B,T", mc.CLS_MEAN_CASES)
def test_cls_mean_bwd_exact(B, T):
    """Three batch strides: the contiguous (B, S, D) gradient (S * D), its [CLS] rows alone (D), and the same rows as the head of the rows of a
    wider NaN-filled buffer (9 * D)."""
    hip = _hip()
    S = 5
    cls_rows = ints((B, D), gen("cls_mean", B, T), -64, 64).to(F32)
    want = mc.cls_mean_ref(cls_rows, T)
    tokens = torch.full((B, S, D), float("nan"))
    tokens[:, 0] = cls_rows
    wide_buf = torch.full((B, 9 * D), float("nan"))
    wide_buf[:, :D] = cls_rows
    layouts = {"contiguous (B, S, D)": tokens.cuda(), "the [CLS] rows alone": cls_rows.cuda(), "head of wider rows": wide_buf.cuda()[:, :D]}
    assert [t.stride(0) for t in layouts.values()] == [S * D, D, 9 * D]
    for what, dx_out in layouts.items():
        assert_same(hip.cls_mean_bwd(dx_out, B, T), want, what)


@pytest.mark.parametrize("n,dt", mc.GELU_CASES, ids=["%d-%s" % (n, DT_NAME[dt]) for n, dt in mc.GELU_CASES])
def test_gelu_bwd_edges(n, dt):
    hip = _hip()
    g = torch.Generator().manual_seed(n % 1000 + 7)
    u, dh = (torch.randn(n, generator=g) * 2).to(dt), torch.randn(n, generator=g).to(dt)
    dh[::7] = 0
    u64 = u.double().requires_grad_(True)
    (torch.nn.functional.gelu(u64) * dh.double()).sum().backward()
    du = torch.full((n + 64,), SENTINEL, dtype=dt, device="cuda")
    dh_dev, u_dev = poisoned_vec(dh, 64, device="cuda"), poisoned_vec(u, 64, device="cuda")
    hip._check(hip.load().alpro_gelu_bwd(hip._ptr(dh_dev), hip._ptr(u_dev), hip._ptr(du), hip.dtype_code(dt), n, hip._stream()), "alpro_gelu_bwd")
    got = du.cpu()
    close(got[:n], u64.grad, *mc.GELU_TOL[dt], "gelu bwd n=%d" % n)
    assert not bool(got[:n][dh == 0].any()), "dh == 0 must give exactly 0"
    assert bool((got[n:] == SENTINEL).all()), "written past n"
    assert torch.equal(hip.gelu_bwd(dh_dev, u_dev).cpu(), got[:n]), "wrapper"
