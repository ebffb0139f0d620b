"""GPU: alpro_attn_temporal_probs against the fp64 softmax inside the bound derived in tests/attn_probs_cases.py (a temporal problem is that file's
problem with batch = groups, L = T and no key bias; only the log-sum-exp layout differs: tests/attn_temporal_probs_cases.py), for every frame
count that takes the unit form (T dividing 32) and the tile form (any other T up to 128), with the log-sum-exp rows of both kernels that write
them in the model (alpro_attn_temporal_fwd, alpro_gemm_qkv_tattn)."""
import functools

import numpy as np
import pytest
import torch

from tests import attn_probs_cases as ac
from tests import attn_temporal_probs_cases as tc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(T, dtype, groups, H=2, peaked=False):
    return tc.peaked_temporal_case(T, dtype, groups, H) if peaked else tc.temporal_case(T, dtype, groups, H)


def _run(case):
    """-> (probabilities, lse in the kernels' chunk layout, attention output) on the device: lse from the temporal forward, as in the model."""
    from alpro_amd import hip
    qkv = torch.from_numpy(case.qkv).cuda().to(ac.TORCH_DTYPE[case.dtype])
    out, lse = hip.attn_temporal(qkv, case.L, case.H, case.scale, want_lse=True)
    return hip.attn_temporal_probs(qkv, lse, case.L, case.H, case.scale), lse, out


def _check(case, p, lse, what=""):
    assert p.shape == (case.batch, case.H, case.L, case.L) and p.dtype == torch.float32 and p.is_contiguous()
    return ac.check(case, p.cpu().numpy(), tc.lse_from_chunks(lse.cpu().numpy(), case.batch, case.L), what)


@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("groups", tc.GROUPS)
@pytest.mark.parametrize("T", tc.FRAMES)
def test_probabilities_and_row_sums_inside_the_bound(T, groups, dtype):
    c = _case(T, dtype, groups)
    p, lse, _ = _run(c)
    _check(c, p, lse)


@pytest.mark.parametrize("T,groups,dtype", [(8, 37, "fp16"), (12, 5, "bf16"), (33, 5, "fp32")])
def test_probabilities_inside_the_bound_twelve_heads(T, groups, dtype):
    c = _case(T, dtype, groups, H=12)
    p, lse, _ = _run(c)
    _check(c, p, lse)


@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("T", (8, 33, 128))
def test_peaked_scores_stay_finite_and_inside_zero_one(T, dtype):
    c = _case(T, dtype, 5, peaked=True)
    p, lse, _ = _run(c)
    pn = p.cpu().numpy()
    assert np.isfinite(pn).all() and pn.max() <= 1.0 and pn.min() >= 0.0
    _check(c, p, lse)


@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-4), ("fp16", 8e-4)])
@pytest.mark.parametrize("T,groups", [(4, 37), (8, 37), (16, 5), (3, 37), (33, 5), (128, 5)])
def test_probabilities_times_values_give_the_attention_output(T, groups, dtype, tol):
    c = _case(T, dtype, groups)
    p, _, out = _run(c)
    ref = out.float().cpu().numpy().astype(np.float64).reshape(groups, T, c.H, 64).transpose(0, 2, 1, 3)     # hip.attn_temporal's output, (groups, H, T, 64)
    got = p.cpu().numpy().astype(np.float64) @ ac.values64(c.qkv, groups, T, c.H)
    err, lim = np.abs(got - ref).max(), tol * np.abs(ref).max()
    print("P @ V vs hip.attn_temporal (T=%d groups=%d %s): max err %.3e, limit %.3e" % (T, groups, dtype, err, lim))
    assert err <= lim


@pytest.mark.parametrize("dtype", ("fp16", "bf16"))
@pytest.mark.parametrize("T", (1, 2, 4, 8, 16))
def test_log_sum_exp_rows_of_the_fused_qkv_launch(T, dtype):
    """q | k | v and lse as alpro_gemm_qkv_tattn writes them (training form) beside alpro_gemm + alpro_attn_temporal_fwd on the same operands: the same
    map bit for bit when the two hand over the same bits, else each inside the bound of its own q | k | v."""
    from alpro_amd import hip
    rows, H, K = 96, 2, 128
    dt = ac.TORCH_DTYPE[dtype]
    rng = np.random.RandomState(4200 + T)
    a = torch.from_numpy(rng.standard_normal((rows, K)).astype(np.float32)).cuda().to(dt)
    w = torch.from_numpy((rng.standard_normal((3 * H * 64, K)) / np.sqrt(K)).astype(np.float32)).cuda().to(dt)
    b = torch.from_numpy(0.1 * rng.standard_normal(3 * H * 64).astype(np.float32)).cuda()
    assert hip.qkv_tattn_ok(a, T)
    _, qkv_f, lse_f = hip.gemm_qkv_tattn(a, w, b, T, H, ac.SCALE, want_qkv=True)
    qkv_g = hip.gemm(a, w, bias=b)
    _, lse_g = hip.attn_temporal(qkv_g, T, H, ac.SCALE, want_lse=True)
    p_f = hip.attn_temporal_probs(qkv_f, lse_f, T, H, ac.SCALE)
    p_g = hip.attn_temporal_probs(qkv_g, lse_g, T, H, ac.SCALE)
    same = torch.equal(qkv_f, qkv_g) and torch.equal(lse_f, lse_g)
    print("T=%d %s: fused q | k | v and lse bitwise equal to the two-launch path's: %s" % (T, dtype, same))
    if same:
        assert torch.equal(p_f, p_g)
    for name, qkv, lse, p in (("fused", qkv_f, lse_f, p_f), ("two-launch", qkv_g, lse_g, p_g)):
        c = tc.case_from_qkv("%s_T%d_%s" % (name, T, dtype), qkv.float().cpu().numpy(), rows // T, T, H, dtype)
        _check(c, p, lse)


@pytest.mark.parametrize("T,groups,dtype", [(8, 37, "bf16"), (33, 5, "fp32"), (2, 37, "fp16")])
def test_two_runs_are_bitwise_equal(T, groups, dtype):
    c = _case(T, dtype, groups)
    a, _, _ = _run(c)
    b, _, _ = _run(c)
    assert torch.equal(a, b)


def test_dropping_the_last_group_changes_nothing_in_front_of_it():
    """Ragged last unit (rows % 32 != 0, the same number of lse chunks with and without the last group): a group's map depends on its own rows only."""
    from alpro_amd import hip
    for T, groups in ((4, 37), (12, 5), (2, 37)):
        c = _case(T, "fp16", groups)
        qkv = torch.from_numpy(c.qkv).cuda().to(torch.float16)
        _, lse = hip.attn_temporal(qkv, T, c.H, c.scale, want_lse=True)
        assert ((groups - 1) * T + 31) // 32 == lse.shape[0]
        p = hip.attn_temporal_probs(qkv, lse, T, c.H, c.scale)
        sub = hip.attn_temporal_probs(qkv[:(groups - 1) * T].contiguous(), lse, T, c.H, c.scale)
        assert torch.equal(sub, p[:groups - 1])


def test_wrapper_refuses_shapes_it_cannot_take():
    from alpro_amd import hip
    c = _case(8, "fp16", 5)
    qkv = torch.from_numpy(c.qkv).cuda().to(torch.float16)
    lse = torch.zeros(2, c.H, 32, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attn_temporal_probs(qkv.cpu(), lse, 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attn_temporal_probs(qkv, lse.cpu(), 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="lse must be"):
        hip.attn_temporal_probs(qkv, lse[:1], 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="lse must be"):
        hip.attn_temporal_probs(qkv, lse.double(), 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="qkv must be"):
        hip.attn_temporal_probs(qkv[:, :128], lse, 8, c.H, c.scale)
    with pytest.raises(RuntimeError, match="rows=40 not a non-negative multiple of T=3"):
        hip.attn_temporal_probs(qkv, lse, 3, c.H, c.scale)
    with pytest.raises(RuntimeError, match="num_frm=0 unsupported"):
        hip.attn_temporal_probs(qkv, lse, 0, c.H, c.scale)
    empty = hip.attn_temporal_probs(qkv[:0], lse[:0], 8, c.H, c.scale)
    assert empty.shape == (0, c.H, 8, 8)
