"""GPU: the video-QA kernels of ABI 22 against fp64 torch -- alpro_gemm_rows_f32 with ReLU and a masked last column tile (any N), its
ReLU-mask backward entry point, and alpro_clip_pool (mean / max / lse over the clips of each question, with the argmax).  Every case runs
twice and must be bitwise equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _u(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float().cuda()


@pytest.mark.parametrize("K", [768, 1536])
@pytest.mark.parametrize("N", [2, 16, 1500, 1504, 3129])
@pytest.mark.parametrize("M", [1, 12, 64, 65, 512])
def test_gemm_rows_relu_any_width(M, N, K):
    from alpro_amd import hip
    a, w, b = _u((M, K), 1 + M), _u((N, K), 2 + N, 0.05), _u((N,), 3 + N, 0.5)
    ref = torch.relu(a.double() @ w.double().t() + b.double())
    # the output sits inside a guard band: nothing at or past column N of a row may be written
    buf = torch.full((M + 1, N + 8), 7.0, dtype=torch.float32, device="cuda")
    out = hip.gemm_rows(a, w, bias=b, act=hip.ACT_RELU, out=buf[:M, :N])
    out2 = hip.gemm_rows(a, w, bias=b, act=hip.ACT_RELU)
    torch.cuda.synchronize()
    assert torch.equal(out, out2), "not bitwise reproducible"
    assert (buf[:M, N:] == 7.0).all() and (buf[M] == 7.0).all(), "wrote past column N / row M"
    err = (out.double() - ref).abs().max().item()
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err
    assert (out >= 0).all()


@pytest.mark.parametrize("N", [2, 1500, 3129])
def test_gemm_rows_plain_ragged_width_with_residual(N):
    """act = none with bias, row scale and residual on a ragged N (the existing epilogue terms, masked at the tail)."""
    from alpro_amd import hip
    M, K = 12, 768
    a, w, b = _u((M, K), 11), _u((N, K), 12, 0.05), _u((N,), 13)
    rs, res = _u((M,), 14), _u((M, N), 15)
    ref = rs.double()[:, None] * (a.double() @ w.double().t() + b.double()) + res.double()
    out = hip.gemm_rows(a, w, bias=b, row_scale=rs, residual=res)
    torch.cuda.synchronize()
    assert (out.double() - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("K", [768, 1536, 3136])
@pytest.mark.parametrize("N", [2, 768, 1500, 1536])
@pytest.mark.parametrize("M", [1, 12, 65, 512])
def test_gemm_rows_relu_mask_backward(M, N, K):
    """dH = (dZ W2) * [H > 0] with the saved forward output H, a third of it exact zeros (ReLU-clipped), read only."""
    from alpro_amd import hip
    a, w = _u((M, K), 21 + M), _u((N, K), 22 + N, 0.05)
    gate = torch.relu(_u((M, N), 23 + K))
    gate[:, ::3] = 0.0
    gate_before = gate.clone()
    ref = (a.double() @ w.double().t()) * (gate.double() > 0)
    out = hip.gemm_rows_relu_mask(a, w, gate)
    out2 = hip.gemm_rows_relu_mask(a, w, gate)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    assert torch.equal(gate, gate_before)
    assert (out[gate == 0] == 0).all()
    err = (out.double() - ref).abs().max().item()
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err


def test_gemm_rows_relu_matches_autograd_of_the_mlp():
    """The answer MLP's backward pieces vs torch autograd in fp64: relu(x W1^T + b1) W2^T + b2, dH through the ReLU mask."""
    from alpro_amd import hip
    M, D, Hd, A = 12, 768, 1536, 1500
    x, w1, b1, w2 = _u((M, D), 31), _u((Hd, D), 32, 0.05), _u((Hd,), 33, 0.5), _u((A, Hd), 34, 0.05)
    dz = _u((M, A), 35)
    h = hip.gemm_rows(x, w1, bias=b1, act=hip.ACT_RELU)
    Ap = 1536
    w2t = torch.nn.functional.pad(w2.t().contiguous(), (0, Ap - A))
    dzp = torch.nn.functional.pad(dz, (0, Ap - A))
    dh = hip.gemm_rows_relu_mask(dzp, w2t, h)
    xd = x.double()
    hd = torch.relu(xd @ w1.double().t() + b1.double())
    ref = (dz.double() @ w2.double()) * (hd > 0)
    torch.cuda.synchronize()
    assert (dh.double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


def _pool_ref(x, C, mode):
    B = x.shape[0] // C
    s = x.double().view(B, C, -1)
    if mode == "mean":
        return s.mean(1)
    if mode == "max":
        return s.amax(1)
    return torch.logsumexp(s, dim=1)


def _logits(B, C, A, kind, seed):
    x = _u((B * C, A), seed, 3.0)
    if kind == "peaked":
        for r in range(B * C):
            x[r, (r * 7919 + seed) % A] += 25.0
    elif kind == "offset":
        x = x + 1000.0 * torch.sign(_u((B * C, 1), seed + 1))
    return x


@pytest.mark.parametrize("kind", ["plain", "peaked", "offset"])
@pytest.mark.parametrize("mode", ["mean", "max", "lse"])
@pytest.mark.parametrize("A", [2, 1500, 3129])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_clip_pool_vs_fp64(C, A, mode, kind):
    from alpro_amd import hip
    B = 5
    x = _logits(B, C, A, kind, 100 * C + A)
    pooled, pred = hip.clip_pool(x, C, mode)
    pooled2, pred2 = hip.clip_pool(x, C, mode)
    torch.cuda.synchronize()
    assert torch.equal(pooled, pooled2) and torch.equal(pred, pred2), "not bitwise reproducible"
    ref = _pool_ref(x, C, mode)
    assert pooled.shape == (B, A) and pred.dtype == torch.int64
    tol = 1e-6 * max(1.0, ref.abs().max().item()) + 1e-6
    err = (pooled.double() - ref).abs().max().item()
    assert err <= tol, (err, tol)
    # the answer is the first index of the pooled row's maximum, exactly; and the fp64 argmax wherever the fp64 top-2 margin is clear of the error
    assert torch.equal(pred, pooled.argmax(-1))
    if A > 1:
        top2 = ref.topk(2, dim=-1).values
        clear = top2[:, 0] - top2[:, 1] > 2 * err + 1e-12
        assert torch.equal(pred[clear], ref.argmax(-1)[clear])


def test_clip_pool_on_a_row_strided_view_and_neg_inf():
    """logits as the first A columns of a padded buffer (how the QA head returns them); lse of all -inf clips is -inf, as torch.logsumexp."""
    from alpro_amd import hip
    B, C, A = 3, 4, 1500
    buf = _u((B * C, 1536), 7)
    buf[0:C, 5] = float("-inf")
    x = buf[:, :A]
    for mode in ("mean", "max", "lse"):
        pooled, pred = hip.clip_pool(x, C, mode)
        ref = _pool_ref(x, C, mode)
        fin = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(pooled), fin)
        assert (pooled.double()[fin] - ref[fin]).abs().max().item() <= 1e-5
        assert torch.equal(pred, ref.argmax(-1))


def test_qa_bindings_refuse_bad_arguments():
    from alpro_amd import hip
    x = _u((6, 16), 1)
    with pytest.raises(ValueError):
        hip.clip_pool(x, 3, "median")
    with pytest.raises(RuntimeError):
        hip.clip_pool(x, 4, "mean")         # 6 rows are not groups of 4 clips
    lib = hip.load()
    pooled = torch.empty((2, 16), device="cuda")
    pred = torch.empty((2,), dtype=torch.int64, device="cuda")
    import ctypes
    for C, mode, msg in ((0, 0, b"C=0"), (3, 7, b"mode 7")):
        rc = lib.alpro_clip_pool(ctypes.c_void_p(x.data_ptr()), 16, ctypes.c_void_p(pooled.data_ptr()), 16, ctypes.c_void_p(pred.data_ptr()), 2, C, 16, mode, None)
        assert rc != 0 and msg in lib.alpro_hip_last_error()
    a, w = _u((4, 64), 2), _u((8, 64), 3)
    with pytest.raises(RuntimeError, match="act"):
        hip.gemm_rows(a, w, act=hip.ACT_GELU_BWD)
    with pytest.raises(RuntimeError, match="K=60"):
        hip.gemm_rows(a[:, :60], w[:, :60])
