"""The data-only LayerNorm backward (alpro_layernorm_bwd / _emit with dgamma == dbeta == NULL: gamma and beta frozen) against the column-sum form
on identical inputs.  It is the same row arithmetic from one text (csrc/layernorm_bwd_kernel.hpp, included twice), and the default build is
deterministic, so dx and the emitted operand rows must be BITWISE equal; nothing outside them may be written.

The C entry points are called directly so that dx and the emit output can sit inside guard regions (the Python wrapper allocates the emit
output itself).  Shapes: the smallest that run the row loops and maps -- 1 row, 9 rows, two workgroups' worth plus one (a workgroup takes 32
rows: 65), and the divided space-time geometries (B, T, N) = (2, 2, 4) and (2, 3, 9)."""
import ctypes

import pytest
import torch

from tests.test_hip_ops import rnd

D = 768
G = 4                 # guard rows in front of and behind every output
SENT = 12345.0        # guard fill (exact in fp32, fp16 and bf16)
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def _guarded(rows, dtype, init=None):
    buf = torch.full((rows + 2 * G, D), SENT, dtype=dtype, device="cuda")
    body = buf[G:G + rows]
    if init is not None:
        body.copy_(init)
    return buf, body


def _guards_ok(buf, rows):
    return bool((buf[:G] == SENT).all()) and bool((buf[G + rows:] == SENT).all())


def _call(hip, dy, dy2, x, gamma, dx, accumulate, dgamma, dbeta, rows, mp, drop, emit_out, em, colsum_pre=None):
    lib = hip.load()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    ws, wsb = hip._reduce_ws(dy.device)
    edt = hip.dtype_code(emit_out.dtype) if emit_out is not None else hip.dtype_code(dy.dtype)
    return lib.alpro_layernorm_bwd_emit(p(dy), hip.dtype_code(dy.dtype), D, p(dy2), p(x), D, p(gamma), 1e-6, p(dx), D, accumulate, p(dgamma), p(dbeta), rows, D,
                                        mp[0], mp[1], mp[2], drop[0], drop[1], p(emit_out), edt, em.get("mode", hip.EMIT_NONE), em.get("T", 0), em.get("N", 0),
                                        p(em.get("scale")), em.get("group", 1), em.get("drop_p", 0.0), em.get("drop_seed", 0), p(colsum_pre), em.get("extra_cls", 0),
                                        ws, wsb, hip._stream())


def _cases(hip):
    """name -> dict(rows, xrows, map (mode, p0, p1), accumulate, dy2, drop (p, seed), emit (dict incl. rows / scale entries) or None)"""
    c = {}
    for rows in (1, 9, 65):
        c["identity_%d" % rows] = dict(rows=rows, xrows=rows, map=(hip.MAP_IDENTITY, 0, 0), accumulate=0)
        c["identity_%d_acc_dy2" % rows] = dict(rows=rows, xrows=rows, map=(hip.MAP_IDENTITY, 0, 0), accumulate=1, dy2=True)
    c["identity_65_dropout"] = dict(rows=65, xrows=65, map=(hip.MAP_IDENTITY, 0, 0), accumulate=0, dy2=True, drop=(0.1, 4711))
    for B, T, N in ((2, 2, 4), (2, 3, 9)):
        S, tag = 1 + N * T, "_B%dT%dN%d" % (B, T, N)
        c["skip_cls" + tag] = dict(rows=B * N * T, xrows=B * S, map=(hip.MAP_SKIP_CLS, N * T, 0), accumulate=1)
        c["skip_cls_noacc" + tag] = dict(rows=B * N * T, xrows=B * S, map=(hip.MAP_SKIP_CLS, N * T, 0), accumulate=0)
        c["frame_tokens" + tag] = dict(rows=B * T * (N + 1), xrows=B * S, map=(hip.MAP_FRAME_TOKENS, T, N), accumulate=1)
        # the three emits as the ViT block's backward uses them (vit.py Block.backward): temporal norm -> ROWS + extra CLS rows, norm2 -> FRAME,
        # norm1 -> SKIP_CLS with the drop-path row scale
        c["emit_rows_extra_cls" + tag] = dict(rows=B * N * T, xrows=B * S, map=(hip.MAP_SKIP_CLS, N * T, 0), accumulate=1,
                                              emit=dict(mode=hip.EMIT_ROWS, rows=B * S, T=T, N=N, nscale=B, group=S, extra_cls=B))
        c["emit_frame" + tag] = dict(rows=B * S, xrows=B * S, map=(hip.MAP_IDENTITY, 0, 0), accumulate=1,
                                     emit=dict(mode=hip.EMIT_FRAME, rows=B * T * (N + 1), T=T, N=N, nscale=B * T))
        c["emit_skip_cls_scaled" + tag] = dict(rows=B * T * (N + 1), xrows=B * S, map=(hip.MAP_FRAME_TOKENS, T, N), accumulate=1,
                                               emit=dict(mode=hip.EMIT_SKIP_CLS, rows=B * N * T, T=T, N=N, nscale=B * N, group=T))
    # the BERT layer's form: fresh dx, a second fp32 gradient stream, the dense-output dropout re-applied to the emitted rows
    c["emit_rows_dropout_dy2"] = dict(rows=65, xrows=65, map=(hip.MAP_IDENTITY, 0, 0), accumulate=0, dy2=True,
                                      emit=dict(mode=hip.EMIT_ROWS, rows=65, drop_p=0.1, drop_seed=77))
    c["emit_rows_9"] = dict(rows=9, xrows=9, map=(hip.MAP_IDENTITY, 0, 0), accumulate=0, emit=dict(mode=hip.EMIT_ROWS, rows=9))
    return c


CASE_NAMES = ["identity_1", "identity_1_acc_dy2", "identity_9", "identity_9_acc_dy2", "identity_65", "identity_65_acc_dy2", "identity_65_dropout",
              "emit_rows_dropout_dy2", "emit_rows_9"] + [k + t for t in ("_B2T2N4", "_B2T3N9")
                                                         for k in ("skip_cls", "skip_cls_noacc", "frame_tokens", "emit_rows_extra_cls", "emit_frame", "emit_skip_cls_scaled")]


def _inputs(hip, case, dt, emit_dt):
    rows, xrows = case["rows"], case["xrows"]
    x = rnd(xrows, D, seed=11, scale=2.0).cuda()
    dy = rnd(rows, D, seed=12).cuda().to(dt)
    dy2 = rnd(rows, D, seed=13).cuda() if case.get("dy2") else None
    gamma = (1.0 + 0.3 * rnd(D, seed=14)).cuda()
    dx0 = rnd(xrows, D, seed=15).cuda()      # what dx holds beforehand: accumulated into, or (rows the map skips) left alone
    em = dict(case.get("emit") or {})
    if em.get("nscale"):
        em["scale"] = (0.5 + rnd(em["nscale"], seed=16).abs()).cuda()
    return x, dy, dy2, gamma, dx0, em


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("dtn", ["fp32", "fp16", "bf16"])
def test_data_only_form_is_bitwise_the_column_sum_form(dtn, name):
    from alpro_amd import hip
    case, dt = _cases(hip)[name], DTYPES[dtn]
    emit_dt = torch.float16 if dt == torch.float32 else dt      # fp32 dy: the <float, f16_t> instantiation (emit_rows_9: <float, float>)
    if name == "emit_rows_9":
        emit_dt = dt
    x, dy, dy2, gamma, dx0, em = _inputs(hip, case, dt, emit_dt)
    got = {}
    canary = torch.full((2, D), SENT, dtype=torch.float32, device="cuda")   # stands where dgamma / dbeta would: passed to neither data-only call
    for form in ("full", "data"):
        dxb, dx = _guarded(case["xrows"], torch.float32, dx0)
        eb, eo = _guarded(em["rows"], emit_dt, torch.zeros(em["rows"], D)) if em else (None, None)   # (rows an emit skips stay at their initial zero in both forms)
        dg, db = (torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")) if form == "full" else (None, None)
        rc = _call(hip, dy, dy2, x, gamma, dx, case["accumulate"], dg, db, case["rows"], case["map"], case.get("drop", (0.0, 0)), eo, em)
        torch.cuda.synchronize()
        assert rc == 0, (form, hip.load().alpro_hip_last_error().decode())
        assert _guards_ok(dxb, case["xrows"]), "%s form wrote outside dx" % form
        assert eb is None or _guards_ok(eb, em["rows"]), "%s form wrote outside the emitted rows" % form
        got[form] = (dx.clone(), None if eo is None else eo.clone(), dg)
    assert bool((canary == SENT).all())
    assert float(got["full"][2].abs().sum()) > 0.0                     # the column-sum form did produce dgamma (the comparison is not vacuous)
    assert not torch.equal(got["full"][0], dx0)                        # ... and dx was written
    assert torch.equal(got["data"][0], got["full"][0]), "dx differs: max |diff| %.3e" % float((got["data"][0] - got["full"][0]).abs().max())
    if em:
        assert float(got["full"][1].float().abs().sum()) > 0.0
        assert torch.equal(got["data"][1], got["full"][1]), "emitted rows differ"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["dgamma", "dbeta"])
def test_one_sided_null_is_refused_and_writes_nothing(which):
    from alpro_amd import hip
    case = _cases(hip)["identity_9"]
    x, dy, dy2, gamma, dx0, em = _inputs(hip, case, torch.float32, torch.float32)
    dxb, dx = _guarded(9, torch.float32, dx0)
    buf = torch.full((D,), SENT, device="cuda")
    rc = _call(hip, dy, None, x, gamma, dx, 0, buf if which == "dgamma" else None, buf if which == "dbeta" else None, 9, case["map"], (0.0, 0), None, {})
    torch.cuda.synchronize()
    msg = hip.load().alpro_hip_last_error().decode()
    assert rc != 0 and "both" in msg and which in msg, (rc, msg)
    assert torch.equal(dx, dx0) and _guards_ok(dxb, 9) and bool((buf == SENT).all())


@pytest.mark.gpu
def test_null_pair_with_colsum_pre_is_refused_by_the_library_and_served_by_the_wrapper():
    """colsum_pre (the temporal_fc bias gradient under the merged projection) needs the column-sum kernel: the C entry point says so, and
    hip.layernorm_bwd(dgamma=None, dbeta=None, emit=dict(colsum_pre=...)) runs it into the throw-away pair -- same dx, rows and colsum_pre."""
    from alpro_amd import hip
    B, T, N = 2, 2, 4
    case = _cases(hip)["emit_skip_cls_scaled_B2T2N4"]
    x, dy, dy2, gamma, dx0, em = _inputs(hip, case, torch.bfloat16, torch.bfloat16)
    cs = torch.zeros(D, device="cuda")
    dx = dx0.clone()
    eo = torch.zeros(em["rows"], D, dtype=torch.bfloat16, device="cuda")
    rc = _call(hip, dy, None, x, gamma, dx, 1, None, None, case["rows"], case["map"], (0.0, 0), eo, em, colsum_pre=cs)
    torch.cuda.synchronize()
    assert rc != 0 and "colsum_pre" in hip.load().alpro_hip_last_error().decode()
    assert torch.equal(dx, dx0) and float(cs.abs().sum()) == 0.0
    res = {}
    for form in ("full", "none"):
        dxf, csf = dx0.clone(), torch.zeros(D, device="cuda")
        dg, db = (torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")) if form == "full" else (None, None)
        _, op = hip.layernorm_bwd(dy, x, gamma, 1e-6, dxf, dg, db, rows=case["rows"], map_mode=case["map"][0], map_p0=T, map_p1=N,
                                  emit=dict(mode=hip.EMIT_SKIP_CLS, rows=em["rows"], dtype=torch.bfloat16, T=T, N=N, scale=em["scale"], group=T, colsum_pre=csf))
        res[form] = (dxf, op, csf)
    torch.cuda.synchronize()
    for a, b in zip(res["none"], res["full"]):
        assert torch.equal(a, b)
    assert float(res["full"][2].abs().sum()) > 0.0
    # one of the pair wanted (gamma trainable, beta frozen): the wanted one is what the full form gives, the other goes to the throw-away buffer
    dxg, dg = dx0.clone(), torch.zeros(D, device="cuda")
    dgf, dbf = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    hip.layernorm_bwd(dy, x, gamma, 1e-6, dxg, dg, None, rows=case["rows"], map_mode=case["map"][0], map_p0=T, map_p1=N)
    hip.layernorm_bwd(dy, x, gamma, 1e-6, dx0.clone(), dgf, dbf, rows=case["rows"], map_mode=case["map"][0], map_p0=T, map_p1=N)
    torch.cuda.synchronize()
    assert torch.equal(dg, dgf) and float(dg.abs().sum()) > 0.0
