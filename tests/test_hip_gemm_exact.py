"""GPU: the GEMM family on arithmetic that is exact in every summation order (tests/gemm_cases.py) -- every element of every case
against the fp64 reference with ZERO tolerance, on all three alpro_gemm kernels and every option setting, inside poisoned surroundings:
operands in NaN-filled buffers (rows at and beyond M and N, padding columns), outputs in sentinel-filled ones whose guard rows and columns
must keep their bits.  The GELU family keeps exact pre-activations and the tolerances of tests/test_hip_ops.py."""
import contextlib

import pytest
import torch

from tests import gemm_cases as gc
from tests.gemm_cases import BF16, F16, F32, F64
from tests.test_hip_ops import OUT_TOL, close

pytestmark = pytest.mark.gpu

NAN_AS = 30000.0          # NaN compares equal to NaN at the same place (the non-finite cases) by mapping both sides to this
GELU_TOL_F32_OF_16 = (2e-5, 2e-4)      # tests/test_hip_ops.py::test_gemm_bias_act: fp32 output of 16-bit operands
WIDE_IN, LDA8 = 64, 8
WIDE_OUT = dict(out=8, res=16, c2=24, side=32)


def _hip():
    from alpro_amd import hip
    hip.load()
    assert (hip.ACT_NONE, hip.ACT_GELU, hip.ACT_RELU, hip.ACT_GELU_BWD, hip.ACT_GELU_SAVE_GRAD, hip.ACT_MUL_SAVED) == (gc.ACT_NONE, gc.ACT_GELU, gc.ACT_RELU, gc.ACT_GELU_BWD, gc.ACT_GELU_SAVE_GRAD, gc.ACT_MUL_SAVED)
    assert (hip.MAP_IDENTITY, hip.MAP_SKIP_CLS, hip.MAP_FRAME_TOKENS, hip.MAP_PATCH_EMBED) == (gc.MAP_IDENTITY, gc.MAP_SKIP_CLS, gc.MAP_FRAME_TOKENS, gc.MAP_PATCH_EMBED)
    return hip


@contextlib.contextmanager
def options(hip, opts):
    """Library options for a block, put back afterwards whatever happens; cu_budget is the per-stream option."""
    with contextlib.ExitStack() as st:
        for k, v in opts:
            if k == "cu_budget":
                hip.set_stream_option("cu_budget", v)
                st.callback(hip.set_stream_option, "cu_budget", -1)
            else:
                st.enter_context(hip.option(k, v))
        yield


def same_bits(got_buf, want_buf):
    g, w = got_buf.detach().cpu(), want_buf
    assert g.dtype == w.dtype and g.shape == w.shape
    return torch.equal(torch.nan_to_num(g.float(), nan=NAN_AS), torch.nan_to_num(w.float(), nan=NAN_AS))


def _geometry(c):
    r0 = 1 if c.layout in ("row1", "lda8_row1") else 0
    in_pad = WIDE_IN if c.layout == "wide_in" else LDA8 if c.layout in ("lda8", "lda8_row1") else 0
    out_pad = WIDE_OUT if c.layout == "wide_out" else dict(out=0, res=0, c2=0, side=0)
    return r0, in_pad, out_pad


def device_inputs(x):
    """The case's operands on the device, each inside its poisoned surroundings (made once per case; launches only read them)."""
    c = x.case
    r0, in_pad, out_pad = _geometry(c)
    r0o = 1 if c.layout == "row1" else 0
    d = dict(a=gc.poisoned(x.a, 300, in_pad, r0, device="cuda"), w=gc.poisoned(x.w, 300, in_pad if c.layout == "wide_in" else 0, 1 if c.layout == "row1" else 0, device="cuda"))
    for k in ("bias", "bias2", "row_scale"):
        t = getattr(x, k)
        d[k] = gc.poisoned_vec(t, 64, device="cuda") if t is not None else None
    d["residual"] = gc.poisoned(x.residual, 8, out_pad["res"], r0o, device="cuda") if x.residual is not None else None
    d["saved"] = gc.poisoned(x.saved, 8, out_pad["c2"], r0o, device="cuda") if x.saved is not None else None
    return d


def launch(hip, x, d, pre_act=None, c2_tiled=False):
    """One alpro_gemm launch of the case into fresh sentinel-filled output buffers -> dict of output VIEWS (buffer: view._base)."""
    c = x.case
    _, _, out_pad = _geometry(c)
    r0o = 1 if c.layout == "row1" else 0
    o = dict(out=gc.poisoned(torch.full((x.out_rows, c.N), gc.SENTINEL, dtype=c.out_dtype), gc.GUARD_ROWS, out_pad["out"], r0o, fill=gc.SENTINEL, device="cuda"))
    kw = {}
    if x.side_rows:
        o["side"] = kw["side"] = gc.poisoned(torch.full((x.side_rows, c.N), gc.SENTINEL, dtype=F32), gc.GUARD_ROWS, out_pad["side"], r0o, fill=gc.SENTINEL, device="cuda")
    if pre_act is not None:
        kw["pre_act"] = pre_act
    elif x.epi.get("c2") in ("copy", "out"):
        o["c2"] = kw["pre_act"] = gc.poisoned(torch.full((c.M, c.N), gc.SENTINEL, dtype=c.dt), gc.GUARD_ROWS, out_pad["c2"], r0o, fill=gc.SENTINEL, device="cuda")
    elif x.saved is not None:
        kw["pre_act"] = d["saved"]
    if x.drop_seed:
        kw.update(drop_p=gc.DROP_P, drop_seed=x.drop_seed)
    if x.row_scale is not None:
        kw.update(row_scale=d["row_scale"], row_scale_group=c.group)
    hip.gemm(d["a"], d["w"], out=o["out"], bias=d["bias"], act=x.act, out_dtype=c.out_dtype, alpha=x.alpha, residual=d["residual"], map_mode=x.map_mode,
             map_p0=x.map_p0, map_p1=x.map_p1, bias2=d["bias2"], c2_tiled=c2_tiled, **kw)
    return o


def expected(x, key, view, ref64=None):
    """The CPU image of an output buffer: the reference rounded once to the buffer's dtype inside the view, the sentinel everywhere else."""
    b = view._base
    r0 = view.storage_offset() // b.shape[1]
    ref = (x.ref[key] if ref64 is None else ref64).to(view.dtype)
    return gc.poisoned(ref, b.shape[0] - r0 - ref.shape[0], b.shape[1] - ref.shape[1], r0, fill=gc.SENTINEL)._base


def tolerance(c, key):
    if c.dt == F32:
        return OUT_TOL[F32]
    return OUT_TOL[c.dt] if (key == "c2" or c.out_dtype != F32) else GELU_TOL_F32_OF_16


def check(x, o, what):
    c = x.case
    for key, view in o.items():
        want = expected(x, key, view)
        if c.exact:
            assert gc.matches(view, x.ref[key], view.dtype) or bool(x.ref[key].isnan().any()), "%s %s: %s differs from the reference rounded once (%d elements)" % (
                c.id, what, key, int((view.detach().cpu().double() != x.ref[key].to(view.dtype).double()).sum()))
            assert same_bits(view._base, want), "%s %s: %s buffer (guards / non-finite row)" % (c.id, what, key)
        else:
            close(view, x.ref[key], *tolerance(c, key), "%s %s %s" % (c.id, what, key))
            got = view._base.detach().cpu().clone()
            r0 = view.storage_offset() // got.shape[1]
            got[r0:r0 + view.shape[0], :view.shape[1]] = 0
            want[r0:r0 + view.shape[0], :view.shape[1]] = 0
            assert torch.equal(got, want), "%s %s: %s guard rows / columns" % (c.id, what, key)


def _tiled_buffer(hip, c):
    rows = hip.gemm_c2_tiled_rows(c.M, c.N, c.K, c.dt)
    assert rows == (c.M + 255) // 256 * 256
    return torch.full((rows, c.N), float("nan"), dtype=c.dt, device="cuda")


@pytest.mark.parametrize("c", gc.GEMM_CASES, ids=[c.id for c in gc.GEMM_CASES])
def test_gemm_exact(c):
    hip = _hip()
    x = gc.build(c)
    d = device_inputs(x)
    first = None
    for opts in c.variants:
        with options(hip, opts):
            if c.route in ("q8", "q8_tail") and c.layout == "tight" and c.M % 16 == 0:
                assert hip.gemm_c2_tiled_rows(c.M, c.N, c.K, c.dt) > 0, "%s: not routed to the 8-phase kernel under %s" % (c.id, opts)
            if c.route == "p256" and opts[:2] == gc.ROUTE_OPTS["q8"] and c.layout == "tight" and not c.group:
                assert hip.gemm_c2_tiled_rows(c.M, c.N, c.K, c.dt) == 0, "%s: meant to be ineligible for the 8-phase kernel" % c.id
            if c.tiled:
                run_tiled(hip, x, d)
                continue
            o1 = launch(hip, x, d)
            o2 = launch(hip, x, d)
        for k in o1:
            assert same_bits(o1[k]._base, o2[k]._base.cpu()), "%s: two runs differ (%s) under %s" % (c.id, k, opts)
        check(x, o1, "under %s" % (opts,))
        if first is None:
            first = o1
        elif not c.exact:      # (exact cases: equal to the reference, therefore to each other)
            for k in o1:
                assert same_bits(o1[k]._base, first[k]._base.cpu()), "%s: %s under %s differs from %s" % (c.id, k, opts, c.variants[0])


def run_tiled(hip, x, d):
    """The tile-layout C2 of the 8-phase kernel: GELU_SAVE_GRAD writes it, MUL_SAVED reads it back; both launches must give the bits of the
    row-layout pair, and MUL_SAVED on the saved factors (data by then: 16-bit values times an integer accumulator stay exact) the reference's."""
    c = x.case
    gs = gc.build(gc.case("q8", c.M, c.N, c.K, c.dt, "same", "gelu_save", tiled=True))
    dg = device_inputs(gs) if c.epi != "gelu_save" else d
    rows = launch(hip, gs, dg)
    u_tile = _tiled_buffer(hip, c)
    tiled = launch(hip, gs, dg, pre_act=u_tile, c2_tiled=True)
    check(gs, rows, "row layout")
    check(gs, tiled, "tile layout")
    assert same_bits(tiled["out"]._base, rows["out"]._base.cpu())
    assert torch.equal(u_tile.view(-1)[:1024].float().sort().values, rows["c2"][:16, :64].reshape(-1).float().sort().values)
    if c.epi == "mul_saved":
        u_rows = rows["c2"]
        m_rows = launch(hip, x, d, pre_act=u_rows)
        m_tile = launch(hip, x, d, pre_act=u_tile, c2_tiled=True)
        assert same_bits(m_tile["out"]._base, m_rows["out"]._base.cpu())
        ref = x.ref["pre"] * u_rows.detach().cpu().to(F64)
        assert float(ref.abs().max()) < 60000.0
        assert gc.matches(m_rows["out"], ref, c.dt)
        assert same_bits(m_rows["out"]._base, expected(x, "out", m_rows["out"], ref))


def test_gemm_strided_outputs_are_addressed_by_their_row_stride():
    """hip.gemm takes ldc / ldr / ldc2 / ld_side from stride(0) of 2-D tensors (the wide_out cases above run through it); what the descriptor
    cannot express is refused."""
    hip = _hip()
    a, w = torch.ones(4, 64, device="cuda"), torch.ones(8, 64, device="cuda")
    buf = torch.zeros(6, 24, device="cuda")
    d, _ = hip.gemm(a, w, out=buf[:4, :8], residual=buf[1:5, 8:16], _desc_only=True)
    assert (d.ldc, d.ldr) == (24, 24)
    d, _ = hip.gemm(a, w, out=torch.zeros(2, 2, 8, device="cuda"), _desc_only=True)
    assert d.ldc == 8
    with pytest.raises(RuntimeError, match="cannot hold rows"):
        hip.gemm(a, w, out=torch.zeros(4, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="cannot hold rows"):
        hip.gemm(a, w, out=torch.zeros(1, 8, device="cuda").expand(4, 8))


# ------------------------------------------------------------------------------------------------ alpro_gemm_batch
def _batch_cases(dt):
    return [gc.case("k128", M, N, K, dt, out, epi) for (M, N, K, epi, out) in gc.BATCH_JOBS]


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_gemm_batch_exact(dt):
    hip = _hip()
    xs = [gc.build(c) for c in _batch_cases(dt)]
    ds = [device_inputs(x) for x in xs]
    for _ in range(2):
        gb = hip.GemmBatch()
        outs = []
        for x, d in zip(xs, ds):
            c = x.case
            o = gc.poisoned(torch.full((c.M, c.N), gc.SENTINEL, dtype=c.out_dtype), gc.GUARD_ROWS, 8, 1, fill=gc.SENTINEL, device="cuda")
            gb.add(d["a"], d["w"], o, bias=d["bias"], alpha=x.alpha, residual=d["residual"], out_dtype=c.out_dtype)
            outs.append(o)
        gb.launch()
        gb.launch()
        for x, o in zip(xs, outs):
            assert gc.matches(o, x.ref["out"], o.dtype), x.case.id
            assert same_bits(o._base, expected(x, "out", o)), x.case.id


def test_gemm_batch_refusals():
    hip = _hip()
    a, w, o = torch.ones(4, 64, device="cuda", dtype=BF16), torch.ones(8, 64, device="cuda", dtype=BF16), torch.zeros(4, 8, device="cuda", dtype=BF16)
    gb = hip.GemmBatch()
    gb.add(a, w, o)
    gb.add(a.half(), w.half(), o.half())
    with pytest.raises(RuntimeError, match="share the operand dtype"):
        gb.launch()
    for kw in (dict(act=hip.ACT_RELU), dict(map_mode=hip.MAP_SKIP_CLS, map_p0=2, out=torch.zeros(8, 8, device="cuda", dtype=BF16))):
        gb = hip.GemmBatch()
        desc, _ = hip.gemm(a, w, **dict(dict(out=o), **kw), _desc_only=True)
        gb._descs.append(desc)
        gb._keep.append((a, w, o, None, None))
        with pytest.raises(RuntimeError, match="plain epilogues only"):
            gb.launch()


# ------------------------------------------------------------------------------------------------ weight-gradient GEMM and column sums
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", gc.TN_SHAPES)
def test_gemm_tn_acc_and_colsums_exact(dt, M, N, K):
    hip = _hip()
    t = gc.tn_inputs(M, N, K, dt)
    padn, padk = (-N) % 8 + 8, (-K) % 8 + 8          # lda / ldb: multiples of 8 beyond the chunk that holds the last column
    a = gc.poisoned(t["a"], 40, padn, 0, device="cuda")
    b = gc.poisoned(t["b"], 40, padk, 0, device="cuda")
    want_c = gc.poisoned(t["ref_c"].to(F32), 4, 8, 1, fill=gc.SENTINEL)._base
    want_cs = gc.poisoned_vec(t["ref_cs"].to(F32), 8, fill=gc.SENTINEL)._base
    for splits in gc.TN_SPLITS:
        for kind in (0, 2):
            for atomic in (False, True):
                with hip.option("tn_splits", splits), hip.option("tn_kind", kind):
                    c = gc.poisoned(t["c0"], 4, 8, 1, fill=gc.SENTINEL, device="cuda")
                    cs = gc.poisoned_vec(t["cs0"], 8, fill=gc.SENTINEL, device="cuda")
                    hip.gemm_tn_acc(a, b, c, colsum=cs, atomic=atomic)
                    what = "tn_splits %d tn_kind %d atomic %s" % (splits, kind, atomic)
                    assert torch.equal(c._base.cpu(), want_c), what
                    assert torch.equal(cs._base.cpu(), want_cs), what + " (colsum)"
                    if not atomic:
                        cs2 = gc.poisoned_vec(t["cs0"], 8, fill=gc.SENTINEL, device="cuda")
                        hip.colsum_tn(a, K, cs2)
                        assert torch.equal(cs2._base, cs._base), what + " (colsum_tn)"
    if N % 8 == 0:
        cs3 = gc.poisoned_vec(t["cs0"], 8, fill=gc.SENTINEL, device="cuda")
        hip.colsum_acc(a, cs3)
        assert torch.equal(cs3._base.cpu(), want_cs), "colsum_acc"
