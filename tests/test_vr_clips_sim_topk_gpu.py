"""GPU: alpro_sim_topk_clips (top-k by pooled similarity, several clips per video) against the cases of tests/sim_topk_clips_cases.py.

mean / max on the exact cases ({-1, 0, 1} * 2^-4 features, one fp32 multiply, fp32 sequential mean): the pooled matrix is known bit for bit and
the result must equal its stable descending sort BIT FOR BIT, values and indices, under every chunk.  lse, and every mode on random unit-norm
features, must stay inside the derived bound of the cases file and return a sorted, duplicate-free list that leaves nothing better out.  For
all three modes every forced chunk gives the bits of the library's choice and two runs are bitwise equal.  With one clip and an exact scale
the result is alpro_sim_topk's, bit for bit."""
import math

import numpy as np
import pytest
import torch

from tests import sim_topk_cases as tc
from tests import sim_topk_clips_cases as cc

pytestmark = pytest.mark.gpu

SIDES = (cc.GALLERY, cc.QUERY)
SIDE_SHAPES = [(side,) + s for side in SIDES for s in cc.shapes(side)]
# (side, lists, ent, n, k, chunk): chunks that span several sub-passes (GALLERY: 9 sub-passes of 73 videos and one of 43; QUERY: 1024 rows), a
# chunk of 96 entries that no sub-pass divides, and 2200 chunks of 32 rows: the four-wave merge and the second merge level
PATH_SHAPES = ((cc.GALLERY, 3, 700, 7, 128, 704), (cc.GALLERY, 35, 300, 3, 16, 96), (cc.QUERY, 2, 5000, 5, 128, 1024), (cc.QUERY, 11, 700, 3, 16, 96),
               (cc.GALLERY, 2, 70400, 2, 16, 32), (cc.QUERY, 2, 70400, 2, 16, 32))


def _run(c, mode, chunk, scale=None):
    from alpro_amd import hip
    val, idx = hip.sim_topk_clips(torch.from_numpy(c.q).cuda(), torch.from_numpy(c.g).cuda(), c.k, c.n, side=c.side, mode=mode,
                                  scale=c.scale if scale is None else scale, chunk=chunk)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == idx.shape == (c.lists, c.k)
    return val.cpu().numpy(), idx.cpu().numpy()


def _same_bits(val, idx, want_val, want_idx, what):
    assert np.array_equal(idx, want_idx), "%s: indices differ at %s" % (what, np.argwhere(idx != want_idx)[:4].tolist())
    assert np.array_equal(val.view(np.int32), want_val.view(np.int32)), "%s: values differ at %s" % (what, np.argwhere(val.view(np.int32) != want_val.view(np.int32))[:4].tolist())


def _check_all_modes(c, chunks):
    for mode in cc.MODES:
        want = cc.expected_topk(cc.pool32(c, mode), c.k) if mode != "lse" and not c.chain.any() else None
        base = None
        for chunk in chunks:
            val, idx = _run(c, mode, chunk)
            what = "%s %s chunk %d" % (c.name, mode, chunk)
            if want is not None:
                _same_bits(val, idx, want[0], want[1], what + " vs the expectation")
            else:
                cc.check_pooled(c, mode, val, idx)
            if base is None:
                base = (val, idx)
            _same_bits(val, idx, base[0], base[1], what + " vs chunk %d" % chunks[0])
        val, idx = _run(c, mode, chunks[0])
        _same_bits(val, idx, base[0], base[1], "%s %s: second run" % (c.name, mode))


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("side,lists,ent,n,k", SIDE_SHAPES)
def test_exact_cases_mean_max_bit_for_bit_and_lse_in_bound_under_every_chunk(side, lists, ent, n, k, kind):
    _check_all_modes(cc.exact_case(side, kind, lists, ent, n, k), cc.CHUNKS)


@pytest.mark.parametrize("side,lists,ent,n,k", SIDE_SHAPES)
def test_random_unit_norm_features_within_the_derived_bound(side, lists, ent, n, k):
    _check_all_modes(cc.random_case(side, lists, ent, n, k), cc.CHUNKS)


@pytest.mark.parametrize("side,lists,ent,n,k,chunk", PATH_SHAPES)
def test_sub_passes_inside_a_chunk_and_merge_levels(side, lists, ent, n, k, chunk):
    _check_all_modes(cc.exact_case(side, "edge_ties", lists, ent, n, k), (chunk, 0))
    _check_all_modes(cc.random_case(side, lists, ent, n, k), (chunk, 0))


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("nq,ng,k", tc.SHAPES)
def test_one_clip_with_an_exact_scale_is_sim_topk_bit_for_bit(kind, nq, ng, k):
    from alpro_amd import hip
    c = tc.exact_case(kind, nq, ng, k)
    q, g = torch.from_numpy(c.q).cuda(), torch.from_numpy(c.g).cuda()
    want_val, want_idx = hip.sim_topk(q, g, k, scale=2.0)
    for side in SIDES:
        for mode in cc.MODES:
            for chunk in (0, 32):
                val, idx = hip.sim_topk_clips(q, g, k, 1, side=side, mode=mode, scale=2.0, chunk=chunk)
                _same_bits(val.cpu().numpy(), idx.cpu().numpy(), want_val.cpu().numpy(), want_idx.cpu().numpy(), "%s %s %s chunk %d" % (c.name, side, mode, chunk))


@pytest.mark.parametrize("side", SIDES)
def test_negative_zero_is_canonicalised(side):
    """A gallery of zeros against negative queries with scale -3: every x_j is a zero of some sign.  mean and max come out as +0.0 (-0.0 is read
    as +0.0 in the order and in out_val) with ascending indices; lse of two zeros is log 2."""
    from alpro_amd import hip
    q = np.full((2, 256), -2.0 ** -4, dtype=np.float32)
    g = np.zeros((40, 256), dtype=np.float32)
    g[7, 3] = -0.0
    rows, ent = (2, 20) if side == cc.GALLERY else (1, 40)
    for mode in cc.MODES:
        val, idx = hip.sim_topk_clips(torch.from_numpy(q).cuda(), torch.from_numpy(g).cuda(), 5, 2, side=side, mode=mode, scale=-3.0, chunk=32)
        val, idx = val.cpu().numpy(), idx.cpu().numpy()
        assert np.array_equal(idx, np.tile(np.arange(5, dtype=np.int32), (rows, 1))), (mode, idx)
        if mode == "lse":
            assert len(set(val.view(np.int32).reshape(-1).tolist())) == 1 and abs(float(val[0, 0]) - math.log(2.0)) <= 4 * 2.0 ** -24, val
        else:
            assert np.array_equal(val.view(np.int32), np.zeros((rows, 5), dtype=np.int32)), (mode, val)


def test_wrapper_refuses_other_dtypes_strides_widths_and_bad_arguments():
    from alpro_amd import hip
    q, g = torch.zeros(6, 256, device="cuda"), torch.zeros(8, 256, device="cuda")
    with pytest.raises(RuntimeError, match="fp32"):
        hip.sim_topk_clips(q.half(), g, 3, 2)
    with pytest.raises(RuntimeError, match="contiguous"):
        hip.sim_topk_clips(q, torch.zeros(8, 512, device="cuda")[:, ::2], 3, 2)
    with pytest.raises(RuntimeError, match="d=128"):
        hip.sim_topk_clips(q[:, :128].contiguous(), g[:, :128].contiguous(), 3, 2)
    for kw, msg in ((dict(clips=0), "clips=0"), (dict(clips=33), "clips=33"), (dict(clips=3), "ng=8"), (dict(clips=4, side="query"), "nq=6"),
                    (dict(k=129), "k=129"), (dict(chunk=48), "chunk=48")):
        a = dict(dict(k=3, clips=2, side="gallery"), **kw)
        with pytest.raises(RuntimeError, match=msg):
            hip.sim_topk_clips(q, g, a["k"], a["clips"], side=a["side"], chunk=a.get("chunk", 0))
    with pytest.raises(ValueError, match="side"):
        hip.sim_topk_clips(q, g, 3, 2, side=2)
    with pytest.raises(ValueError, match="median"):
        hip.sim_topk_clips(q, g, 3, 2, mode="median")
