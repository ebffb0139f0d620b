"""GPU: alpro_sim_topk (similarity + top-k without the matrix) against the cases of tests/sim_topk_cases.py.

Exact cases ({-1, 0, 1} * 2^-4 features: every similarity is known bit for bit and ties are everywhere) must match the fp64 expectation --
value descending, gallery index ascending, -inf / -1 behind ng -- BIT FOR BIT, under every chunk size, and every forced chunk must give the
bits of the library's own choice.  Random unit-norm features must stay inside the worst-case bound of a 256-term fp32 chain and return a
sorted, duplicate-free list that leaves nothing better out.  Further shapes force the paths the six shapes of the issue do not reach: the
four-wave merge (more than 512 lists per query), the second merge level (more than 2048 lists) and sub-passes inside a chunk (chunk > 512).
"""
import numpy as np
import pytest
import torch

from tests import sim_topk_cases as tc

pytestmark = pytest.mark.gpu

# (nq, ng, k, chunk): 514 lists -> the four-wave merge; 2049 lists -> two merge levels; chunks of 1024 rows -> running lists over two sub-passes
PATH_SHAPES = ((3, 16417, 16, 32), (2, 65537, 16, 32), (3, 5000, 128, 1024), (67, 1000, 32, 1024), (40, 1500, 100, 1504))


def _run(q, g, k, scale, chunk):
    from alpro_amd import hip
    val, idx = hip.sim_topk(torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda(), k, scale=scale, chunk=chunk)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == idx.shape == (q.shape[0], k)
    return val.cpu().numpy(), idx.cpu().numpy()


def _same_bits(val, idx, want_val, want_idx, what):
    assert np.array_equal(idx, want_idx), "%s: indices differ at %s" % (what, np.argwhere(idx != want_idx)[:4].tolist())
    assert np.array_equal(val.view(np.int32), want_val.view(np.int32)), "%s: values differ at %s" % (what, np.argwhere(val.view(np.int32) != want_val.view(np.int32))[:4].tolist())


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("nq,ng,k", tc.SHAPES)
def test_exact_cases_match_fp64_bit_for_bit_under_every_chunk(kind, nq, ng, k):
    c = tc.exact_case(kind, nq, ng, k)
    base = None
    for chunk in tc.CHUNKS:
        val, idx = _run(c.q, c.g, c.k, c.scale, chunk)
        _same_bits(val, idx, c.val, c.idx, "%s chunk %d vs fp64" % (c.name, chunk))
        if base is None:
            base = (val, idx)
        _same_bits(val, idx, base[0], base[1], "%s chunk %d vs chunk 0" % (c.name, chunk))


@pytest.mark.parametrize("nq,ng,k", tc.SHAPES)
def test_random_unit_norm_features_within_the_chain_bound(nq, ng, k):
    c = tc.random_case(nq, ng, k)
    base = None
    for chunk in tc.CHUNKS:
        val, idx = _run(c.q, c.g, c.k, 1.0, chunk)
        tc.check_random(c, val, idx)
        if base is None:
            base = (val, idx)
        _same_bits(val, idx, base[0], base[1], "%s chunk %d vs chunk 0" % (c.name, chunk))


@pytest.mark.parametrize("nq,ng,k,chunk", PATH_SHAPES)
def test_merge_levels_and_sub_passes(nq, ng, k, chunk):
    c = tc.exact_case("edge_ties", nq, ng, k)
    val, idx = _run(c.q, c.g, c.k, c.scale, chunk)
    _same_bits(val, idx, c.val, c.idx, "%s chunk %d vs fp64" % (c.name, chunk))
    r = tc.random_case(nq, ng, k)
    val, idx = _run(r.q, r.g, r.k, 1.0, chunk)
    tc.check_random(r, val, idx)
    v0, i0 = _run(r.q, r.g, r.k, 1.0, 0)
    _same_bits(val, idx, v0, i0, "%s chunk %d vs chunk 0" % (r.name, chunk))


def test_negative_zero_is_canonicalised_and_scale_is_one_multiply():
    """A gallery of zeros against negative queries: every product is -0.0 or +0.0; the values come out as +0.0 * scale and the indices ascend."""
    q = np.full((2, 256), -2.0 ** -4, dtype=np.float32)
    g = np.zeros((40, 256), dtype=np.float32)
    g[7, 3] = -0.0
    val, idx = _run(q, g, 5, -3.0, 32)
    assert np.array_equal(idx, np.tile(np.arange(5, dtype=np.int32), (2, 1)))
    assert np.array_equal(val.view(np.int32), np.full((2, 5), np.float32(0.0) * np.float32(-3.0), dtype=np.float32).view(np.int32))


def test_wrapper_refuses_other_dtypes_strides_and_widths():
    from alpro_amd import hip
    q, g = torch.zeros(4, 256, device="cuda"), torch.zeros(9, 256, device="cuda")
    with pytest.raises(RuntimeError, match="fp32"):
        hip.sim_topk(q.half(), g, 3)
    with pytest.raises(RuntimeError, match="contiguous"):
        hip.sim_topk(q, torch.zeros(9, 512, device="cuda")[:, ::2], 3)
    with pytest.raises(RuntimeError, match="d=128"):
        hip.sim_topk(q[:, :128].contiguous(), g[:, :128].contiguous(), 3)
    with pytest.raises(RuntimeError, match="k=129"):
        hip.sim_topk(q, g, 129)
    with pytest.raises(RuntimeError, match="chunk=48"):
        hip.sim_topk(q, g, 3, chunk=48)
