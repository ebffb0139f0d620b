"""GPU: alpro_vit_final_pool_mode and alpro_vit_final_pool_mode_bwd (final LayerNorm + the 'spatial' / 'none' pooling of
TimeSformer.forward_features, csrc/core.hip and csrc/backward.hip) against torch fp64 on the same fp32 operands, with fp32 / fp16 / bf16 outputs.

The five (B, T, N) cases: the smallest possible; odd everything; the real frame geometry (8 x 196) at tiny B; N = 33, above and not a multiple of
the spatial kernel's 8 waves (and of their two-rows-per-trip stride 16); B = 5 with T = 2, whose row counts (165 token rows, 15 / 170 output rows)
are no multiple of the 4 rows a workgroup of the row kernels takes.  Tolerances are those the suite already applies to alpro_vit_final_pool
(TOL32, OUT_TOL) and to alpro_layernorm_bwd (BWD_DX, BWD_DG).  Outputs are written through the C entry points into buffers with sentinel-filled
guard rows on both sides; every call runs three times and must repeat bit for bit."""
import pytest
import torch

from tests.test_hip_bwd_ops import _determinism
from tests.test_hip_ops import DTYPES, OUT_TOL, _hip, close, rnd
from tests.test_hip_rowwise_stress import BWD_DG, BWD_DX, TOL32

pytestmark = pytest.mark.gpu

D, EPS = 768, 1e-6
GUARD, SENTINEL = 4, -7.0
CASES = [(1, 1, 1), (2, 3, 9), (3, 8, 196), (2, 5, 33), (5, 2, 16)]
MODES = ["spatial", "none"]


def pool64(y, mode, B, T, N):
    """y (B, 1 + N*T, D), patch (n, t) at row 1 + n*T + t -> the reference's pooled tensor (vit.py:484-499)."""
    cls, p = y[:, :1], y[:, 1:].reshape(B, N, T, D).permute(0, 2, 1, 3)   # (B, T, N, D)
    if mode == "temporal":
        return torch.cat([cls, p.mean(1)], 1)
    if mode == "spatial":
        return torch.cat([cls, p.mean(2)], 1)
    return torch.cat([cls.unsqueeze(1).expand(B, T, 1, D), p], 2)


def operands(B, T, N, seed):
    S = 1 + N * T
    x = rnd(B, S, D, seed=seed) * 2 + 0.3
    return x, 1 + 0.1 * rnd(D, seed=seed + 1), 0.1 * rnd(D, seed=seed + 2)


def guarded(rows, dtype):
    """(whole buffer, the (rows, D) window between GUARD sentinel rows on either side)"""
    buf = torch.full((rows + 2 * GUARD, D), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + rows]


def guards_intact(buf, what):
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), what + ": a guard row was written"


def code(hip, mode):
    return {"temporal": hip.POOL_TEMPORAL, "spatial": hip.POOL_SPATIAL, "none": hip.POOL_NONE}[mode]


@pytest.fixture(scope="module")
def refs():
    """fp64 references per (case, mode), computed once: outputs, and gradients under the fixed dout."""
    cache = {}

    def get(B, T, N, mode):
        key = (B, T, N, mode)
        if key not in cache:
            x, g, b = operands(B, T, N, seed=100 + 7 * N + T)
            x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, g, b))
            out = pool64(torch.nn.functional.layer_norm(x64, (D,), g64, b64, EPS), mode, B, T, N)
            dout = rnd(*out.shape, seed=200 + N)
            (out * dout.double()).sum().backward()
            cache[key] = dict(x=x, g=g, b=b, out=out.detach(), dout=dout, dx=x64.grad, dg=g64.grad, db=b64.grad)
        return cache[key]
    return get


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,T,N", CASES)
@pytest.mark.parametrize("dt", DTYPES)
def test_final_pool_mode_forward(refs, dt, B, T, N, mode):
    hip = _hip()
    lib = hip.load()
    r = refs(B, T, N, mode)
    x, g, b = r["x"].cuda(), r["g"].cuda(), r["b"].cuda()
    rows_out = r["out"].numel() // D
    runs = []
    for _ in range(3):
        b32, o32 = guarded(rows_out, torch.float32)
        bt, ot = guarded(rows_out, dt) if dt != torch.float32 else (None, None)
        hip._check(lib.alpro_vit_final_pool_mode(hip._ptr(x), hip._ptr(g), hip._ptr(b), EPS, hip._ptr(o32), hip._ptr(ot), hip.dtype_code(dt), code(hip, mode),
                                                 x.numel() // D, B, T, N, D, hip._stream()), "alpro_vit_final_pool_mode")
        guards_intact(b32, "%s out32" % mode)
        if bt is not None:
            guards_intact(bt, "%s out %s" % (mode, dt))
        runs.append((o32.clone(), ot.clone() if ot is not None else None))
    ref = r["out"].reshape(rows_out, D)
    close(runs[0][0], ref, *TOL32, "%s out32 (B, T, N) = %s" % (mode, (B, T, N)))
    if dt != torch.float32:
        close(runs[0][1], ref, *OUT_TOL[dt], "%s out %s" % (mode, dt))
    for o32, ot in runs[1:]:
        assert torch.equal(o32, runs[0][0]) and (ot is None or torch.equal(ot, runs[0][1])), "%s forward is not bit-reproducible" % mode
    # the tensor-level wrapper: the same launch on its own buffers, in the reference's output shape
    w32, wt = hip.vit_final_pool_mode(x, g, b, EPS, B, T, N, dt, code(hip, mode))
    assert tuple(w32.shape) == tuple(r["out"].shape) == tuple(wt.shape) and wt.dtype == dt
    assert torch.equal(w32.view(-1, D), runs[0][0]) and (dt == torch.float32 or torch.equal(wt.view(-1, D), runs[0][1]))


@pytest.mark.parametrize("B,T,N", CASES)
def test_mode_entry_point_in_temporal_mode_is_alpro_vit_final_pool(refs, B, T, N):
    hip = _hip()
    r = refs(B, T, N, "temporal")
    x, g, b = r["x"].cuda(), r["g"].cuda(), r["b"].cuda()
    a32, at = hip.vit_final_pool(x, g, b, EPS, B, T, N, torch.float16)
    m32, mt = hip.vit_final_pool_mode(x, g, b, EPS, B, T, N, torch.float16, hip.POOL_TEMPORAL)
    assert torch.equal(a32, m32) and torch.equal(at, mt)
    close(m32, r["out"], *TOL32, "temporal through the mode entry point")


@pytest.mark.parametrize("mode", MODES + ["temporal"])
@pytest.mark.parametrize("B,T,N", CASES)
@pytest.mark.parametrize("dt", DTYPES)
def test_final_pool_mode_backward(refs, dt, B, T, N, mode):
    """dt: the dtype of the emitted operand rows (dx itself, dgamma and dbeta are fp32).  dgamma / dbeta are ACCUMULATED into what the buffers
    hold; the emitted rows are dx times the per-clip scale."""
    hip = _hip()
    lib = hip.load()
    r = refs(B, T, N, mode)
    S = 1 + N * T
    x, g, dout = r["x"].cuda(), r["g"].cuda(), r["dout"].cuda()
    dg0, db0 = rnd(D, seed=31), rnd(D, seed=32)
    scale = (0.5 + torch.arange(B, dtype=torch.float32) / 4).cuda()
    runs = []
    for _ in range(3):
        bx, dx = guarded(B * S, torch.float32)
        be, em = guarded(B * S, dt)
        dg, db = dg0.cuda(), db0.cuda()
        ws, wsb = hip._reduce_ws(x.device)
        hip._check(lib.alpro_vit_final_pool_mode_bwd(hip._ptr(dout), hip._ptr(x), hip._ptr(g), EPS, hip._ptr(dx), hip._ptr(dg), hip._ptr(db), code(hip, mode), B * S, B, T, N,
                                                     D, hip._ptr(em), hip.dtype_code(dt), hip._ptr(scale), S, ws, wsb, hip._stream()), "alpro_vit_final_pool_mode_bwd")
        guards_intact(bx, "%s dx" % mode)
        guards_intact(be, "%s emitted rows" % mode)
        runs.append((dx.clone(), em.clone(), dg, db))
    dx, em, dg, db = runs[0]
    what = "%s bwd (B, T, N) = %s " % (mode, (B, T, N))
    close(dx, r["dx"].reshape(-1, D), *BWD_DX, what + "dx")
    close(dg, dg0.double() + r["dg"], *BWD_DG, what + "dgamma")
    close(db, db0.double() + r["db"], *BWD_DG, what + "dbeta")
    sc_rows = scale.cpu().double().repeat_interleave(S)[:, None]
    close(em, r["dx"].reshape(-1, D) * sc_rows, OUT_TOL[dt][0] + BWD_DX[0], BWD_DX[1] * float(scale.max()), what + "emitted rows")   # (as test_hip_rowwise_stress checks emits)
    for other in runs[1:]:
        assert all(torch.equal(a, b_) for a, b_ in zip(other, runs[0])), what + "is not bit-reproducible"
    # the tensor-level wrapper (no emit: one tensor back; with emit: the pair), and the atomic form of the column sums (determinism off)
    dg, db = dg0.cuda(), db0.cuda()
    wdx = hip.vit_final_pool_mode_bwd(dout, x, g, EPS, dg, db, B, T, N, code(hip, mode))
    assert torch.equal(wdx.view(-1, D), dx) and torch.equal(dg, runs[0][2]) and torch.equal(db, runs[0][3])
    with _determinism(hip, False):
        dg, db = dg0.cuda(), db0.cuda()
        adx, aem = hip.vit_final_pool_mode_bwd(dout, x, g, EPS, dg, db, B, T, N, code(hip, mode), emit=dict(dtype=dt, scale=scale, group=S))
    assert torch.equal(adx.view(-1, D), dx) and torch.equal(aem, em)
    close(dg, dg0.double() + r["dg"], *BWD_DG, what + "dgamma (atomics)")
    close(db, db0.double() + r["db"], *BWD_DG, what + "dbeta (atomics)")


def test_wrapper_refuses_shapes_that_do_not_fit():
    hip = _hip()
    B, T, N = 2, 3, 9
    x, g, b = (t.cuda() for t in operands(B, T, N, seed=5))
    with pytest.raises(RuntimeError, match="rows=55 is not B"):
        hip.vit_final_pool_mode(x.view(-1, D)[:55].contiguous(), g, b, EPS, B, T, N, torch.float32, hip.POOL_SPATIAL)
    with pytest.raises(RuntimeError, match="dout is"):
        hip.vit_final_pool_mode_bwd(torch.zeros(B, 1 + N, D, device="cuda"), x, g, EPS, torch.zeros(D).cuda(), torch.zeros(D).cuda(), B, T, N, hip.POOL_SPATIAL)
    with pytest.raises(RuntimeError, match="do not cover"):
        hip.vit_final_pool_mode_bwd(torch.zeros(B, 1 + T, D, device="cuda"), x, g, EPS, torch.zeros(D).cuda(), torch.zeros(D).cuda(), B, T, N, hip.POOL_SPATIAL,
                                    emit=dict(dtype=torch.float16, scale=torch.ones(1).cuda(), group=1 + N * T))
