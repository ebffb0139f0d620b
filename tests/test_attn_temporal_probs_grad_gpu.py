"""GPU: alpro_attn_temporal_probs_grad against the fp64 expectations inside the bounds derived in tests/attn_probs_grad_cases.py (a temporal
problem is that file's problem with batch = groups, L = T and no key bias: tests/attn_temporal_probs_grad_cases.py), for every frame count that
takes the unit form (T dividing 32) and the tile form (any other T up to 128), 12 heads, both dctx scales; the bitwise identities (P is
alpro_attn_temporal_probs' value, one output against the pair, reruns, the power-of-two scale under fp32 operands); and the softmax backward
restated from the returned P and G against alpro_attn_temporal_bwd, inside the tolerance tests/test_hip_bwd_ops.py holds that kernel to.
The lse rows come from the temporal forward, as in the model."""
import numpy as np
import pytest
import torch

from tests import attn_probs_cases as ac
from tests import attn_probs_grad_cases as gc
from tests import attn_temporal_probs_cases as tc
from tests import attn_temporal_probs_grad_cases as tg

pytestmark = pytest.mark.gpu

BWD_TOL = {"fp32": (2e-4, 2e-5), "bf16": (3e-2, 3e-2), "fp16": (5e-3, 5e-3)}   # (rtol, atol): tests/test_hip_bwd_ops.py GRAD_TOL


def _dev(g):
    dt = ac.TORCH_DTYPE[g.case.dtype]
    return torch.from_numpy(g.case.qkv).cuda().to(dt), torch.from_numpy(g.dctx).cuda().to(dt)


def _lse(qkv, c):
    from alpro_amd import hip
    out, lse = hip.attn_temporal(qkv, c.L, c.H, c.scale, want_lse=True)
    return out, lse


def _run_checked(g, what=""):
    """One case through the kernel: shapes, both bounds, and every bitwise identity that needs no second case.  -> (grad, cam, lse)."""
    from alpro_amd import hip
    c = g.case
    qkv, dctx = _dev(g)
    _, lse = _lse(qkv, c)
    grad, cam = hip.attn_temporal_probs_grad(qkv, dctx, lse, c.L, c.H, c.scale, grad_scale=g.grad_scale)
    for t in (grad, cam):
        assert t.shape == (c.batch, c.H, c.L, c.L) and t.dtype == torch.float32 and t.is_contiguous()
    gc.check_grad(g, grad.cpu().numpy(), what)
    gc.check_cam(g, cam.cpu().numpy(), tc.lse_from_chunks(lse.cpu().numpy(), c.batch, c.L), what)
    # P is alpro_attn_temporal_probs' value and the product is one fp32 multiply
    assert torch.equal(cam, hip.attn_temporal_probs(qkv, lse, c.L, c.H, c.scale) * grad.clamp(min=0))
    # one output alone, the other order, a second run: the same bits
    assert torch.equal(hip.attn_temporal_probs_grad(qkv, dctx, lse, c.L, c.H, c.scale, want=("cam",), grad_scale=g.grad_scale), cam)
    assert torch.equal(hip.attn_temporal_probs_grad(qkv, dctx, lse, c.L, c.H, c.scale, want="grad", grad_scale=g.grad_scale), grad)
    cam2, grad2 = hip.attn_temporal_probs_grad(qkv, dctx, lse, c.L, c.H, c.scale, want=("cam", "grad"), grad_scale=g.grad_scale)
    assert torch.equal(cam2, cam) and torch.equal(grad2, grad)
    return grad, cam, lse


@pytest.mark.parametrize("dtype", tg.DTYPES)
@pytest.mark.parametrize("groups", tg.GROUPS)
@pytest.mark.parametrize("T", tg.FRAMES)
def test_gradient_and_cam_inside_the_bounds_and_the_bitwise_identities(T, groups, dtype):
    g = tg.temporal_grad_case(T, dtype, groups)
    grad, cam, _ = _run_checked(g)
    assert float(grad.abs().max()) > 0 and float(cam.max()) > 0
    small = tg.temporal_grad_case(T, dtype, groups, small=True)
    del g
    grad_s, cam_s, _ = _run_checked(small, " (2^-10 dctx, grad_scale 2^10)")
    if dtype == "fp32":   # exact products of a power-of-two multiple, one exact rescale: the unscaled run's bits
        assert torch.equal(grad_s, grad) and torch.equal(cam_s, cam)


@pytest.mark.parametrize("dtype", tg.DTYPES)
@pytest.mark.parametrize("T", (8, 33, 128))
def test_peaked_scores(T, dtype):
    g = tg.temporal_grad_case(T, dtype, 5, peaked=True)
    grad, cam, _ = _run_checked(g, " peaked")
    assert bool(torch.isfinite(cam).all()) and float(cam.min()) >= 0
    _run_checked(tg.temporal_grad_case(T, dtype, 5, peaked=True, small=True), " peaked (2^-10 dctx, grad_scale 2^10)")


@pytest.mark.parametrize("dtype", tg.DTYPES)
@pytest.mark.parametrize("T,groups", [(3, 37), (8, 37), (33, 5)])
def test_the_maps_reproduce_the_temporal_backward(T, groups, dtype):
    """dS = P o (G - rowsum(P o G)) in fp64 from the returned P and G -> dq, dk, dv against hip.attn_temporal_bwd's."""
    from alpro_amd import hip
    g = tg.temporal_grad_case(T, dtype, groups)
    c = g.case
    qkv, dctx = _dev(g)
    out, lse = _lse(qkv, c)
    grad = hip.attn_temporal_probs_grad(qkv, dctx, lse, T, c.H, c.scale, want="grad")
    p = hip.attn_temporal_probs(qkv, lse, T, c.H, c.scale)
    want = tg.dqkv_from_maps(c, g.dctx, p.cpu().numpy(), grad.cpu().numpy())
    got = hip.attn_temporal_bwd(qkv, out, dctx, lse, T, c.H, c.scale).float().cpu().numpy().astype(np.float64)
    rtol, atol = BWD_TOL[dtype]
    frac = np.abs(got - want) / (atol + rtol * np.abs(want))
    for i, name in enumerate("qkv"):
        f = frac.reshape(groups * T, 3, -1)[:, i]
        print("[tprobs_grad] T=%d groups=%d %s d%s from the maps vs attn_temporal_bwd: worst error / tolerance %.3f" % (T, groups, dtype, name, f.max()))
    assert frac.max() <= 1.0 and np.abs(want).max() > 0


def test_dropping_the_last_group_changes_nothing_in_front_of_it():
    """Ragged last unit (rows % 32 != 0): a group's maps depend on its own rows only."""
    from alpro_amd import hip
    for T, groups in ((4, 37), (12, 5), (2, 37)):
        g = tg.temporal_grad_case(T, "fp16", groups, H=2)
        c = g.case
        qkv, dctx = _dev(g)
        _, lse = _lse(qkv, c)
        assert ((groups - 1) * T + 31) // 32 == lse.shape[0]
        grad, cam = hip.attn_temporal_probs_grad(qkv, dctx, lse, T, c.H, c.scale)
        n = (groups - 1) * T
        sg, sc = hip.attn_temporal_probs_grad(qkv[:n].contiguous(), dctx[:n].contiguous(), lse, T, c.H, c.scale)
        assert torch.equal(sg, grad[:groups - 1]) and torch.equal(sc, cam[:groups - 1])


def test_wrapper_refuses_shapes_it_cannot_take():
    from alpro_amd import hip
    g = tg.temporal_grad_case(8, "fp16", 5, H=2)
    c = g.case
    qkv, dctx = _dev(g)
    lse = torch.zeros(2, c.H, 32, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attn_temporal_probs_grad(qkv, dctx.cpu(), lse, 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attn_temporal_probs_grad(qkv, dctx, lse.cpu(), 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="lse must be"):
        hip.attn_temporal_probs_grad(qkv, dctx, lse[:1], 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="lse must be"):
        hip.attn_temporal_probs_grad(qkv, dctx, lse.double(), 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="qkv must be"):
        hip.attn_temporal_probs_grad(qkv[:, :128], dctx, lse, 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="dctx must be"):
        hip.attn_temporal_probs_grad(qkv, dctx[:-1], lse, 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="dctx must be"):
        hip.attn_temporal_probs_grad(qkv, dctx.float(), lse, 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="dctx must be"):
        hip.attn_temporal_probs_grad(qkv, dctx.t().contiguous().t(), lse, 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="rows=40 not a non-negative multiple of T=3"):
        hip.attn_temporal_probs_grad(qkv, dctx, lse, 3, c.H, c.scale)
    with pytest.raises(RuntimeError, match="num_frm=0 unsupported"):
        hip.attn_temporal_probs_grad(qkv, dctx, lse, 0, c.H, c.scale)
    eg, ec = hip.attn_temporal_probs_grad(qkv[:0], dctx[:0], lse[:0], 8, c.H, c.scale)
    assert eg.shape == ec.shape == (0, c.H, 8, 8)
