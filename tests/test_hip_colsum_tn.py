"""alpro_colsum_tn: the bias gradient of a Linear whose weight is frozen, with the BITS the weight-gradient GEMM (alpro_gemm_tn_acc_ws) gives it.

The kernel restates that GEMM's order of additions -- token ranges, the k-tiles' turns, the 8-token fragments, the reduce tree -- so the oracle is
the GEMM's own colsum output on the same dY, and the comparison is torch.equal.  Shapes: the smallest that take each path of the plan -- one
stage; a token count that is no multiple of 32; several token ranges (9 tiles split from ~130 stages on); 12 k-tiles taking turns (K = 3072);
several column tiles (N = 2304, 3072); the LM head's row-strided (M, 30522) view; a forced split (the tn_splits option)."""
import pytest
import torch

from tests.test_hip_ops import rnd

pytestmark = pytest.mark.gpu

SHAPES = [(32, 768, 768), (9, 768, 768), (203, 768, 768), (4099, 768, 768), (1500, 768, 3072), (1030, 3072, 768), (777, 2304, 768), (60, 30522, 768)]


def _both(hip, M, N, K, dt):
    ld = (N + 63) // 64 * 64
    a = (rnd(M, ld, seed=M + N) * 0.5).cuda().to(dt)[:, :N]        # (the LM head's gradient is the first N columns of a padded buffer)
    b = rnd(M, K, seed=K).cuda().to(dt)
    init = rnd(N, seed=7).cuda()
    ref, got = init.clone(), init.clone()
    hip.gemm_tn_acc(a, b, torch.zeros(N, K, device="cuda"), colsum=ref)
    hip.colsum_tn(a, K, got)
    torch.cuda.synchronize()
    return ref, got, init


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_colsum_tn_has_the_weight_gradient_gemms_bits(M, N, K, dt):
    from alpro_amd import hip
    ref, got, init = _both(hip, M, N, K, dt)
    assert not torch.equal(ref, init)
    assert torch.equal(got, ref), "max |diff| %.3e in %d columns" % (float((got - ref).abs().max()), int((got != ref).sum()))


@pytest.mark.parametrize("splits", [1, 3, 5])
def test_colsum_tn_follows_a_forced_token_split(splits):
    from alpro_amd import hip
    with hip.option("tn_splits", splits):
        ref, got, _ = _both(hip, 1500, 768, 768, torch.bfloat16)
    assert torch.equal(got, ref)


def test_colsum_tn_refuses_fp32_rows():
    from alpro_amd import hip
    with pytest.raises(RuntimeError, match="16-bit"):
        hip.colsum_tn(torch.zeros(8, 768, device="cuda"), 768, torch.zeros(768, device="cuda"))
