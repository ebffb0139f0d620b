"""The three entry points of the ViT block against each other: Block.forward (in place, no-grad), Block.forward_train (out of place) and
Block.forward_cls (CLS-only tail) state the same block (vit.py:146-212), so a change to one stage must show in all of them -- with the merged
temporal projection and with the two Linears as written (merge_temporal_proj = False, whose forward and forward_cls no other test runs).

One 768-wide block of tests/test_vit_attn_dropout.py in eval mode on at most 38 tokens per clip."""
import pytest
import torch

from tests.test_hip_ops import rnd
from tests.test_vit_attn_dropout import D, TOL, _block, _fix_drop_path

CLS_TOL = {"fp32": 2e-5, "fp16": 4e-3}   # tests/test_model_parity.py::test_forward_cls_equals_cls_row_of_forward_features: |err| <= tol * max(1, max|full|)


@pytest.mark.gpu
@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
@pytest.mark.parametrize("B,T,W", [(2, 2, 4), (2, 3, 3)])   # 64 temporal rows (the fused temporal launch takes them), L = 17 | T = 3: the windowed temporal kernel, L = 10
def test_block_entry_points_agree(B, T, W, mode, merge):
    from alpro_amd import config as rt
    from alpro_amd.modeling.timesformer.vit import join_cls_chain
    N = W * W
    blk = _block(0.0).eval()
    blk.merge_temporal_proj = merge
    x = rnd(B, 1 + N * T, D, seed=620).cuda()
    with rt.use_compute_dtype(mode), torch.no_grad():
        # (ii) forward_cls is the CLS row of forward.  forward_cls is the eval-mode path and applies no drop-path scale, so this half runs with the
        # module's own eval-mode _drop (no scales); the 16-bit CLS row of forward is the one it restates, hence use_cls_precise("0")
        with rt.use_cls_precise("0"):
            full = blk(x.clone(), B, T, W)
            cls = blk.forward_cls(x.clone(), B, T, W)
        err, lim = float((cls - full[:, 0]).abs().max()), CLS_TOL[mode] * max(1.0, float(full.abs().max()))
        print("[block paths %s merge=%d T=%d] forward_cls vs forward[:, 0]: err %.3e limit %.3e" % (mode, merge, T, err, lim))
        assert cls.shape == (B, D) and err <= lim, (err, lim)
        # (i) forward and forward_train, under the fixed drop-path scales of the attention-dropout tests (one clip's MLP branch dropped)
        _fix_drop_path(blk, B, T, N)
        y = blk(x.clone(), B, T, W)
        join_cls_chain(x.device)  # the precise-CLS chain of the in-place forward runs on its side stream by default
        out = blk.forward_train(x.clone(), B, T, W)[0]
        err, lim = float((y - out).abs().max()), 2 * TOL[mode] * float(out.abs().max())
        print("[block paths %s merge=%d T=%d] forward vs forward_train: err %.3e limit %.3e" % (mode, merge, T, err, lim))
        assert err <= lim, (err, lim)
    torch.cuda.synchronize()
