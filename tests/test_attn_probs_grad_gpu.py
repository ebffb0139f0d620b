"""GPU: alpro_attn_probs_grad against the fp64 expectations inside the bounds derived in tests/attn_probs_grad_cases.py (computed from each
case's inputs and the observed error of the forward kernel's log-sum-exp rows; no tuned constant), its bitwise properties (CAM = P * relu(G)
with alpro_attn_probs' P, windows are slices, reruns, the power-of-two grad_scale), and a cross-check of the returned P and G against the
existing flash-style backward: dS = P o (G - rowsum(P o G)) rebuilt in fp64 gives alpro_attn_bwd's dq | dk | dv."""
import functools

import numpy as np
import pytest
import torch

from tests import attn_probs_cases as ac
from tests import attn_probs_grad_cases as gc
from tests.test_attn_probs_gpu import WINDOWS

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(L, dtype, H=2, bias="mixed", peaked=False, small=False):
    c = ac.peaked_case(L, dtype) if peaked else ac.random_case(L, dtype, H=H, bias=bias)
    return gc.with_dctx(c, small=small)


def _dev(g):
    c = g.case
    dt = ac.TORCH_DTYPE[c.dtype]
    qkv = torch.from_numpy(c.qkv).cuda().to(dt)
    dctx = torch.from_numpy(g.dctx).cuda().to(dt)
    kb = None if c.bias is None else torch.from_numpy(c.bias).cuda()
    return qkv, dctx, kb


def _run(g, want=("grad", "cam"), q_range=None, k_range=None, grad_scale=None):
    """-> (what hip.attn_probs_grad returns, lse, attention output): lse from the forward kernel, as in the model."""
    from alpro_amd import hip
    c = g.case
    qkv, dctx, kb = _dev(g)
    out, lse = hip.attn(qkv, c.batch, c.L, c.H, c.scale, kb, want_lse=True)
    res = hip.attn_probs_grad(qkv, dctx, lse, c.batch, c.L, c.H, c.scale, kb, q_range=q_range, k_range=k_range, want=want,
                              grad_scale=g.grad_scale if grad_scale is None else grad_scale)
    return res, lse, out


def _check(g):
    from alpro_amd import hip
    c = g.case
    (grad, cam), lse, _ = _run(g)
    shape = (c.batch, c.H, c.L, c.L)
    for t in (grad, cam):
        assert t.shape == shape and t.dtype == torch.float32 and t.is_contiguous()
    gc.check_grad(g, grad.cpu().numpy())
    gc.check_cam(g, cam.cpu().numpy(), lse.cpu().numpy())
    # CAM is alpro_attn_probs' P times relu(G), one fp32 multiply: bit for bit what torch makes of the two tensors
    qkv, _, kb = _dev(g)
    p = hip.attn_probs(qkv, lse, c.batch, c.L, c.H, c.scale, kb)
    assert torch.equal(cam, p * grad.clamp(min=0))
    return grad, cam


@pytest.mark.parametrize("dtype", ac.DTYPES)
@pytest.mark.parametrize("L", ac.LENGTHS)
def test_gradient_and_cam_inside_their_bounds_and_cam_is_p_times_relu_g(L, dtype):
    _check(_case(L, dtype))


@pytest.mark.parametrize("L,dtype,H,bias", [(33, "fp16", 12, "mixed"), (65, "fp32", 2, "none"), (300, "bf16", 2, "none"), (237, "fp16", 2, "none")])
def test_twelve_heads_and_no_bias(L, dtype, H, bias):
    _check(_case(L, dtype, H=H, bias=bias))


@pytest.mark.parametrize("dtype", ac.DTYPES)
@pytest.mark.parametrize("L", (65, 300))
def test_peaked_scores(L, dtype):
    grad, cam = _check(_case(L, dtype, peaked=True))
    assert float(cam.max()) > 0.0


@pytest.mark.parametrize("dtype", ac.DTYPES)
@pytest.mark.parametrize("L", (33, 237))
def test_small_dctx_with_a_power_of_two_grad_scale(L, dtype):
    """dctx = 2^-10 x the same draws and grad_scale = 2^10 -- a loss-scaled backward seen from the kernel: inside the same bounds; fp32 operands
    (where the scaled dctx is exactly 2^-10 x the unscaled one and every product and partial sum scales with it) bit for bit the unscaled result;
    16-bit operands, whose scaled dctx was rounded separately, within limG of the expectation of the unscaled case."""
    g0, g1 = _case(L, dtype), _case(L, dtype, small=True)
    grad1, cam1 = _check(g1)
    (grad0, cam0), _, _ = _run(g0)
    if dtype == "fp32":
        assert torch.equal(grad0, grad1) and torch.equal(cam0, cam1)
    else:
        err = np.abs(grad1.cpu().numpy().astype(np.float64) - g1.g64)
        assert (err <= gc.bound_grad(g1)).all()


@pytest.mark.parametrize("dtype", ("fp32", "fp16"))
@pytest.mark.parametrize("L", (237, 300))
def test_windows_single_outputs_and_reruns_are_bitwise(L, dtype):
    g = _case(L, dtype)
    (grad, cam), _, _ = _run(g)
    (grad2, cam2), _, _ = _run(g)
    assert torch.equal(grad, grad2) and torch.equal(cam, cam2)                       # a rerun
    only_cam, _, _ = _run(g, want=("cam",))
    only_grad, _, _ = _run(g, want="grad")
    swapped, _, _ = _run(g, want=("cam", "grad"))
    assert torch.is_tensor(only_cam) and torch.equal(only_cam, cam) and torch.equal(only_grad, grad)
    assert torch.equal(swapped[0], cam) and torch.equal(swapped[1], grad)
    B, H = g.case.batch, g.case.H
    for (qa, qb), (ka, kb) in WINDOWS:
        qb, kb = L if qb is None else qb, L if kb is None else kb
        (wg, wc), _, _ = _run(g, q_range=(qa, qb), k_range=(ka, kb))
        assert wg.shape == wc.shape == (B, H, qb - qa, kb - ka) and wg.is_contiguous() and wc.is_contiguous()
        assert torch.equal(wg, grad[:, :, qa:qb, ka:kb]) and torch.equal(wc, cam[:, :, qa:qb, ka:kb]), ((qa, qb), (ka, kb))
        w1, _, _ = _run(g, want=("cam",), q_range=(qa, qb), k_range=(ka, kb))
        assert torch.equal(w1, wc)


# alpro_attn_bwd against fp64 in tests/test_hip_bwd_ops.py: close(d, ref, rtol, atol * max(1, max |ref|)) with these (rtol, atol) per dtype
GRAD_TOL = {"fp32": (2e-4, 2e-5), "bf16": (3e-2, 3e-2), "fp16": (5e-3, 5e-3)}


@pytest.mark.parametrize("dtype", ac.DTYPES)
@pytest.mark.parametrize("L", (65, 237))
def test_p_and_g_rebuild_the_existing_backward(L, dtype):
    """dS = P o (G - rowsum(P o G)), dq = scale dS k, dk = scale dS^T q, dv = P^T dO in fp64 from the RETURNED P and G, against hip.attn_bwd on
    the same buffers (bias 'pad': no all-masked sequence -- there every score sits at -10000, fp32 resolves it to 2^-10, and the relative 1e-3
    on P that results is the bound test's business)."""
    from alpro_amd import hip
    from tests.test_hip_bwd_ops import GRAD_TOL as BWD_TOL
    assert BWD_TOL[ac.TORCH_DTYPE[dtype]] == GRAD_TOL[dtype]
    g = _case(L, dtype, bias="pad")
    c = g.case
    qkv, dctx, kb = _dev(g)
    ctx, lse = hip.attn(qkv, c.batch, L, c.H, c.scale, kb, want_lse=True)
    p = hip.attn_probs(qkv, lse, c.batch, L, c.H, c.scale, kb).cpu().numpy().astype(np.float64)
    grad = hip.attn_probs_grad(qkv, dctx, lse, c.batch, L, c.H, c.scale, kb, want="grad").cpu().numpy().astype(np.float64)
    dqkv = hip.attn_bwd(qkv, ctx, dctx, lse, c.batch, L, c.H, c.scale, kb).float().cpu().numpy().astype(np.float64).reshape(c.batch, L, 3, c.H, 64)
    x = c.qkv.astype(np.float64).reshape(c.batch, L, 3, c.H, 64)
    q, k = x[:, :, 0].transpose(0, 2, 1, 3), x[:, :, 1].transpose(0, 2, 1, 3)
    ds = p * (grad - (p * grad).sum(axis=-1, keepdims=True))
    want = (c.scale * ds @ k, c.scale * ds.transpose(0, 1, 3, 2) @ q, p.transpose(0, 1, 3, 2) @ gc.dctx_rows64(g.dctx, c.batch, L, c.H))
    rtol, atol = GRAD_TOL[dtype]
    for i, name in enumerate("qkv"):
        got, ref = dqkv[:, :, i].transpose(0, 2, 1, 3), want[i]
        lim = atol * max(1.0, np.abs(ref).max()) + rtol * np.abs(ref)
        err = np.abs(got - ref)
        print("d%s from P and G vs hip.attn_bwd (L=%d %s): max err %.3e, worst error / limit %.3f (max |ref| %.3e)" % (name, L, dtype, err.max(), (err / lim).max(), np.abs(ref).max()))
        assert (err <= lim).all()


def test_wrapper_refuses_shapes_and_windows_it_cannot_take():
    from alpro_amd import hip
    g = _case(33, "fp16")
    c = g.case
    qkv, dctx, kb = _dev(g)
    lse = torch.zeros(c.batch, c.H, c.L, device="cuda")
    for kw, msg in ((dict(q_range=(0, 34)), "q0=0 nq=34"), (dict(k_range=(5, 5)), "nk=0"), (dict(k_range=(-1, 4)), "k0=-1"), (dict(q_range=(9, 3)), "nq=-6")):
        with pytest.raises(RuntimeError, match=msg):
            hip.attn_probs_grad(qkv, dctx, lse, c.batch, c.L, c.H, c.scale, kb, **kw)
    with pytest.raises(RuntimeError, match="dctx must be"):
        hip.attn_probs_grad(qkv, dctx.float(), lse, c.batch, c.L, c.H, c.scale, kb)
    with pytest.raises(RuntimeError, match="dctx must be"):
        hip.attn_probs_grad(qkv, dctx[:, :64], lse, c.batch, c.L, c.H, c.scale, kb)
    with pytest.raises(RuntimeError, match="lse must be"):
        hip.attn_probs_grad(qkv, dctx, lse[:, :1], c.batch, c.L, c.H, c.scale, kb)
    with pytest.raises(RuntimeError, match="qkv must be"):
        hip.attn_probs_grad(qkv[:, :128], dctx, lse, c.batch, c.L, c.H, c.scale, kb)
    with pytest.raises(RuntimeError, match="key_bias must be"):
        hip.attn_probs_grad(qkv, dctx, lse, c.batch, c.L, c.H, c.scale, kb[:, :4])
