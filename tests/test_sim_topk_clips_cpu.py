"""CPU: the host side of the multi-clip retrieval search -- alpro_sim_topk_clips' ABI surface and argument checks (every check sits in front of
the first HIP call, so placeholder addresses are never read), the self-check of the case builders (tests/sim_topk_clips_cases.py), and the
refusal of an unknown score_agg_func by the evaluation functions before they touch the model."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import sim_topk_clips_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("alpro_sim_topk_clips", "alpro_sim_topk_clips_workspace_bytes")
SIDES = (cc.GALLERY, cc.QUERY)


def test_new_entry_points_are_exported_and_declared_under_abi_22():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    lib = hip.load()
    for name in NEW:
        assert name in hip.EXPORTS and re.search(r"\b(int|size_t)\s+%s\s*\(" % name, hdr) and hasattr(lib, name), name
    assert "#define ALPRO_TOPK_MAX_CLIPS 32" in hdr and hip.TOPK_MAX_CLIPS == 32
    assert "enum { ALPRO_TOPK_CLIPS_GALLERY = 0, ALPRO_TOPK_CLIPS_QUERY = 1 };" in hdr and hip.TOPK_CLIPS_SIDES == {"gallery": 0, "query": 1}
    assert "#define ALPRO_HIP_ABI_VERSION 22" in hdr and hip.ABI_VERSION == 22 == lib.alpro_hip_abi_version()


def test_bad_arguments_are_refused_with_a_message_that_names_the_value():
    from alpro_amd import hip
    lib = hip.load()
    p = ctypes.c_void_p(4096)
    good = dict(nq=6, ng=100, d=256, k=10, clips=2, side=0, mode=0, chunk=0)

    def size(a):
        return lib.alpro_sim_topk_clips_workspace_bytes(a["nq"], a["ng"], a["k"], a["clips"], a["side"], a["chunk"])

    def call(ws_bytes=None, ws=p, **kw):
        a = dict(good, **kw)
        need = size(a)
        return lib.alpro_sim_topk_clips(p, a["nq"], p, a["ng"], a["d"], a["k"], 1.0, a["clips"], a["side"], a["mode"], a["chunk"], p, p, ws,
                                        need if ws_bytes is None else ws_bytes, None)

    assert size(good) > 0
    # the size query returns 0 and says why; the call refuses the same arguments
    for kw, msg in ((dict(clips=0), "clips=0"), (dict(clips=33, ng=99), "clips=33"), (dict(ng=101), "ng=101"), (dict(side=1, nq=7), "nq=7"),
                    (dict(side=2), "side=2"), (dict(k=129), "k=129"), (dict(chunk=48), "chunk=48"), (dict(k=0), "k=0"), (dict(nq=0), "nq=0"),
                    (dict(ng=0), "ng=0"), (dict(chunk=-32), "chunk=-32"), (dict(side=-1), "side=-1")):
        assert size(dict(good, **kw)) == 0, kw
        assert msg in lib.alpro_hip_last_error().decode(), (kw, lib.alpro_hip_last_error())
        assert call(**kw) != 0, kw
        assert msg in lib.alpro_hip_last_error().decode(), (kw, lib.alpro_hip_last_error())
    for kw, msg in ((dict(d=128), "d=128"), (dict(mode=3), "mode=3")):
        assert call(**kw) != 0 and msg in lib.alpro_hip_last_error().decode(), (kw, lib.alpro_hip_last_error())
    need = size(good)
    assert call(ws_bytes=need - 1) != 0 and "workspace_bytes=%d" % (need - 1) in lib.alpro_hip_last_error().decode()
    assert call(ws=ctypes.c_void_p(4096 + 64)) != 0 and "256-byte aligned" in lib.alpro_hip_last_error().decode()


def test_workspace_counts_lists_and_gallery_entries_not_rows():
    from alpro_amd import hip
    lib = hip.load()
    # min(k, chunk) keys of 8 bytes per (list, chunk of entries), 256-byte granules.  GALLERY: 700 videos of 7 clips in chunks of 32 videos;
    # QUERY: 11 videos (33 query rows) are 11 lists over 257 gallery rows
    assert lib.alpro_sim_topk_clips_workspace_bytes(3, 700 * 7, 128, 7, 0, 32) == (3 * 22 * 32 * 8 + 255) // 256 * 256
    assert lib.alpro_sim_topk_clips_workspace_bytes(33, 257, 10, 3, 1, 64) == (11 * 5 * 10 * 8 + 255) // 256 * 256
    # one clip: the plan of alpro_sim_topk
    for nq, ng, k, chunk in ((33, 257, 10, 64), (3, 5000, 128, 0), (1000, 100000, 16, 0)):
        for side in (0, 1):
            assert lib.alpro_sim_topk_clips_workspace_bytes(nq, ng, k, 1, side, chunk) == lib.alpro_sim_topk_workspace_bytes(nq, ng, k, chunk)


def test_wrapper_refuses_cpu_tensors_and_unknown_names():
    from alpro_amd import hip
    q, g = torch.zeros(4, 256), torch.zeros(8, 256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.sim_topk_clips(q, g, 3, 2)
    with pytest.raises(ValueError, match="median"):
        hip.sim_topk_clips(q, g, 3, 2, mode="median")
    with pytest.raises(ValueError, match="side"):
        hip.sim_topk_clips(q, g, 3, 2, side="both")


def test_evaluation_refuses_an_unknown_score_agg_func_before_touching_the_model():
    from alpro_amd import retrieval_eval as re_
    msg = "Invalid value for pool_method, got median, expect one of"      # the text of qa_eval.inference_qa
    with pytest.raises(ValueError, match=msg):
        re_.inference_retrieval_cached(None, None, None, None, None, num_clips=3, score_agg_func="median")
    with pytest.raises(ValueError, match=msg):
        re_.score_all_pairs(None, None, None, None, num_clips=3, score_agg_func="median")
    with pytest.raises(ValueError, match=msg):
        re_.rerank_retrieval(None, None, None, None, None, None, 2, num_clips=3, score_agg_func="median")
    with pytest.raises(ValueError, match=msg):      # and with one clip, where the function would make no difference
        re_.score_all_pairs(None, None, None, None, score_agg_func="median")


def _brute(case, mode):
    """the pooled fp32 value of every (list, entry) by scalar loops over the rows of q and g -- no cube, no reshape"""
    out = np.zeros((case.lists, case.ent), dtype=np.float32)
    sc = np.float32(case.scale)
    for i in range(case.lists):
        for e in range(case.ent):
            xs = []
            for j in range(case.n):
                qi, gi = (i, e * case.n + j) if case.side == cc.GALLERY else (i * case.n + j, e)
                s = np.float32(0.0)
                for t in range(256):
                    s = np.float32(s + case.q[qi, t] * case.g[gi, t])
                xs.append(np.float32(s * sc))
            if mode == "max":
                out[i, e] = max(xs)
            else:
                acc = np.float32(0.0)
                for x in xs:
                    acc = np.float32(acc + x)
                out[i, e] = acc / np.float32(case.n)
    return out


@pytest.mark.parametrize("side", SIDES)
def test_builders_agree_with_a_brute_force_loop_on_a_hand_sized_case(side):
    c = cc.exact_case(side, "random", 2, 5, 3, 4)
    assert c.q.shape == ((2, 256) if side == cc.GALLERY else (6, 256)) and c.g.shape == ((15, 256) if side == cc.GALLERY else (5, 256))
    for mode in ("mean", "max"):
        p = cc.pool32(c, mode)
        assert p.dtype == np.float32 and np.array_equal(p.view(np.int32), _brute(c, mode).view(np.int32)), mode
        assert np.abs(p.astype(np.float64) - cc.pool64(c, mode)).max() <= cc.bound(c, mode).max()
        val, idx = cc.expected_topk(p, c.k)
        for i in range(2):      # the stable descending sort, written out
            want = sorted(range(5), key=lambda e: (-float(p[i, e]), e))[:4]
            assert idx[i].tolist() == want and np.array_equal(val[i], p[i, want])
    lse = cc.pool64(c, "lse")
    for i in range(2):
        for e in range(5):
            assert abs(lse[i, e] - math.log(sum(math.exp(x) for x in c.x64[i, e]))) < 1e-12
    # fewer entries than k: the tail
    val, idx = cc.expected_topk(cc.pool32(c, "max"), 7)
    assert (idx[:, 5:] == -1).all() and np.isneginf(val[:, 5:]).all() and (idx[:, :5] >= 0).all()
    # -0.0 is read as +0.0: it ties with +0.0 and the smaller index goes first, the value comes out as +0.0
    val, idx = cc.expected_topk(np.array([[0.0, -0.0, -1.0]], dtype=np.float32), 3)
    assert idx.tolist() == [[0, 1, 2]] and val.view(np.int32).tolist() == [[0, 0, np.float32(-1.0).view(np.int32)]]


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("side", SIDES)
def test_exact_case_builders_hold_what_they_claim(side, kind):
    grid = {np.float32(v * 2.0 ** -4) for v in (-1, 0, 1)}
    for lists, ent, n, k in cc.shapes(side):
        c = cc.exact_case(side, kind, lists, ent, n, k)
        per_ent = n if side == cc.GALLERY else 1
        assert c.q.shape == (lists * (1 if side == cc.GALLERY else n), 256) and c.g.shape == (ent * per_ent, 256) and c.q.dtype == c.g.dtype == np.float32
        assert set(np.unique(c.q)) <= grid and set(np.unique(c.g)) <= grid
        assert c.s64.shape == (lists, ent, n) and np.abs(c.s64 * 256).max() <= 256 and np.array_equal(c.s64 * 256, np.round(c.s64 * 256))
        # the cube is the clip-by-clip product: entry e, clip j
        e, j = ent - 1, n - 1
        qi, gi = (0, e * n + j) if side == cc.GALLERY else (j, e)
        assert c.s64[0, e, j] == float(c.q[qi].astype(np.float64) @ c.g[gi].astype(np.float64))
        ents = c.g.reshape(ent, per_ent * 256)
        if kind == "dup" and ent >= 6:
            m = ent // 3
            assert np.array_equal(ents[:m], ents[m:2 * m]) and np.array_equal(ents[:m], ents[2 * m:3 * m])
        if kind == "equal":
            assert (ents == ents[0]).all()
        for mode in ("mean", "max"):
            val, idx = cc.expected_topk(cc.pool32(c, mode), k)
            m = min(k, ent)
            assert (idx[:, m:] == -1).all() and np.isneginf(val[:, m:]).all()
            assert ((val[:, :m - 1] > val[:, 1:m]) | ((val[:, :m - 1] == val[:, 1:m]) & (idx[:, :m - 1] < idx[:, 1:m]))).all()
            if kind == "equal":
                assert np.array_equal(idx[:, :m], np.tile(np.arange(m, dtype=np.int32), (lists, 1)))
            if kind == "edge_ties":   # list 0's best candidates are exactly the edge entries, in index order: ties on both sides of every edge
                es = [e for e in cc.edges(side, n) if e < ent]
                for e in es:
                    assert np.array_equal(ents[e - 1], ents[e])
                want = sorted({x for e in es for x in (e - 1, e)})[:m]
                assert idx[0, :len(want)].tolist() == want and len(set(val[0, :len(want)].tolist())) <= 1, (c.name, mode)


@pytest.mark.parametrize("side", SIDES)
def test_mean_and_max_disagree_on_every_multi_clip_shape(side):
    """A kernel that ignores `mode` or `clips` must not pass: on the random exact cases the expected INDICES of mean and max differ in some row,
    and both differ from the indices of clip 0 alone.  (A gallery of one entry has one possible index list; there the values differ.)"""
    for lists, ent, n, k in cc.shapes(side):
        if n == 1:
            continue
        c = cc.exact_case(side, "random", lists, ent, n, k)
        mean, mx = cc.pool32(c, "mean"), cc.pool32(c, "max")
        clip0 = c.s64[:, :, 0].astype(np.float32) * np.float32(c.scale)
        if ent == 1:
            assert not np.array_equal(mean, mx) and not np.array_equal(mean, clip0), c.name      # (some clip is the maximum: here it may be clip 0)
            continue
        i_mean, i_max, i_0 = (cc.expected_topk(p, k)[1] for p in (mean, mx, clip0))
        assert (i_mean != i_max).any() and (i_mean != i_0).any() and (i_max != i_0).any(), c.name


def test_check_pooled_accepts_fp64_and_refuses_broken_results():
    c = cc.random_case(cc.GALLERY, 7, 40, 3, 8)
    assert np.allclose(np.linalg.norm(c.q, axis=1), 1, atol=1e-6) and np.allclose(np.linalg.norm(c.g, axis=1), 1, atol=1e-6)
    for mode in cc.MODES:
        b = cc.bound(c, mode)
        assert 1e-6 < b.max() < 1e-3, (mode, b.max())           # |x| <= 1 / 0.07: a few fp32 ulps of 14, far below the gaps of random values
        val, idx = cc.expected_topk(cc.pool64(c, mode).astype(np.float32), c.k)
        cc.check_pooled(c, mode, val, idx)
        for breaker in ("swap", "repeat", "miss", "other_mode"):
            v, i = val.copy(), idx.copy()
            if breaker == "swap":
                v[0, [0, 1]], i[0, [0, 1]] = v[0, [1, 0]], i[0, [1, 0]]
            elif breaker == "repeat":
                v[0, 1], i[0, 1] = v[0, 0], i[0, 0]
            elif breaker == "miss":
                order = np.argsort(-cc.pool64(c, mode)[0], kind="stable")
                v[0, :-1], i[0, :-1] = v[0, 1:], i[0, 1:]
                v[0, -1], i[0, -1] = np.float32(cc.pool64(c, mode)[0, order[c.k]]), order[c.k]
            else:
                other = "max" if mode != "max" else "mean"
                v, i = cc.expected_topk(cc.pool64(c, other).astype(np.float32), c.k)
            with pytest.raises(AssertionError):
                cc.check_pooled(c, mode, v, i)
