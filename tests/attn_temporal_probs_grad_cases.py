"""Cases for alpro_attn_temporal_probs_grad (the gradient w.r.t. the temporal attention probabilities of the visual encoder and their Grad-CAM map).
Shared by tests/test_attn_temporal_probs_grad_gpu.py and tests/test_attn_temporal_probs_grad_cpu.py; not collected itself, numpy on the CPU only.

A temporal problem over `groups` groups of T consecutive rows IS a problem of tests/attn_probs_cases.py with batch = groups, L = T and no key bias
(tests/attn_temporal_probs_cases.py builds it), and dctx is the same (rows, H*64) matrix, row g*T + t.  So with_dctx, the fp64 expectations and
the derived bounds bound_grad / bound_cam / check_grad / check_cam of tests/attn_probs_grad_cases.py apply unchanged: no new tolerance here, only
the builders and, for the cross-check against alpro_attn_temporal_bwd, the softmax backward stated from P and G.
"""
import numpy as np

from tests import attn_probs_cases as ac
from tests import attn_probs_grad_cases as gc
from tests import attn_temporal_probs_cases as tc

FRAMES, GROUPS, DTYPES = tc.FRAMES, tc.GROUPS, tc.DTYPES
H = 12


def temporal_grad_case(T, dtype, groups, H=H, peaked=False, small=False):
    """-> attn_probs_grad_cases.GradCase of the temporal problem (batch = groups, L = T, no key bias)."""
    case = tc.peaked_temporal_case(T, dtype, groups, H) if peaked else tc.temporal_case(T, dtype, groups, H)
    return gc.with_dctx(case, small=small)


def dqkv_from_maps(case, dctx, p, g):
    """The attention backward from the two maps, fp64: dS = P o (G - rowsum(P o G)), dq = scale dS k, dk = scale dS^T q, dv = P^T dctx
    -> (rows, 3*H*64), laid out like q | k | v.  p, g: (groups, H, T, T)."""
    groups, T, Hn = case.batch, case.L, case.H
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    rows = lambda third: case.qkv.astype(np.float64).reshape(groups, T, 3, Hn, 64)[:, :, third].transpose(0, 2, 1, 3)   # noqa: E731  (groups, H, T, 64)
    q, k = rows(0), rows(1)
    d = gc.dctx_rows64(dctx, groups, T, Hn)
    ds = p * (g - (p * g).sum(-1, keepdims=True))
    parts = (case.scale * (ds @ k), case.scale * (ds.transpose(0, 1, 3, 2) @ q), p.transpose(0, 1, 3, 2) @ d)
    return np.stack([x.transpose(0, 2, 1, 3) for x in parts], axis=2).reshape(groups * T, 3 * Hn * 64)
