"""CPU: the host side of the two-stage retrieval search -- alpro_sim_topk's ABI surface and argument checks (every check sits in front of the
first HIP call, so placeholder addresses are never read), the self-check of the exact case builders (tests/sim_topk_cases.py), and
rerank_metrics against the metrics the REFERENCE's eval_retrieval computed (tests/golden/retrieval_eval_T2_V5.npz)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import sim_topk_cases as tc
from tests.conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("alpro_sim_topk", "alpro_sim_topk_workspace_bytes")


def test_new_entry_points_are_exported_and_declared_under_abi_22():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    lib = hip.load()
    for name in NEW:
        assert name in hip.EXPORTS and re.search(r"\b(int|size_t)\s+%s\s*\(" % name, hdr) and hasattr(lib, name), name
    assert "#define ALPRO_TOPK_MAX_K 128" in hdr and hip.TOPK_MAX_K == 128
    assert "#define ALPRO_HIP_ABI_VERSION 22" in hdr and hip.ABI_VERSION == 22 == lib.alpro_hip_abi_version()


def test_bad_arguments_are_refused_with_a_message_that_names_the_value():
    from alpro_amd import hip
    lib = hip.load()
    p = ctypes.c_void_p(4096)
    good = dict(nq=4, ng=100, d=256, k=10, chunk=0)

    def call(ws_bytes=None, **kw):
        a = dict(good, **kw)
        need = lib.alpro_sim_topk_workspace_bytes(a["nq"], a["ng"], a["k"], a["chunk"])
        return lib.alpro_sim_topk(p, a["nq"], p, a["ng"], a["d"], a["k"], 1.0, a["chunk"], p, p, p, need if ws_bytes is None else ws_bytes, None), need

    for kw, msg in ((dict(d=128), "d=128"), (dict(k=0), "k=0"), (dict(k=129), "k=129"), (dict(chunk=48), "chunk=48"), (dict(nq=0), "nq=0"),
                    (dict(chunk=-32), "chunk=-32"), (dict(ng=0), "ng=0")):
        rc, _ = call(**kw)
        assert rc != 0, kw
        assert msg in lib.alpro_hip_last_error().decode(), (kw, lib.alpro_hip_last_error())
    need = lib.alpro_sim_topk_workspace_bytes(4, 100, 10, 0)
    assert need >= 4 * 10 * 8 and need % 256 == 0
    rc, _ = call(ws_bytes=need - 1)
    assert rc != 0 and "workspace_bytes=%d" % (need - 1) in lib.alpro_hip_last_error().decode(), lib.alpro_hip_last_error()
    # the size query refuses the same arguments (0 bytes) and says why
    assert lib.alpro_sim_topk_workspace_bytes(4, 100, 129, 0) == 0 and "k=129" in lib.alpro_hip_last_error().decode()
    # a workspace that is not 256-byte aligned
    rc = lib.alpro_sim_topk(p, 4, p, 100, 256, 10, 1.0, 0, p, p, ctypes.c_void_p(4096 + 64), need, None)
    assert rc != 0 and "256-byte aligned" in lib.alpro_hip_last_error().decode()


def test_workspace_grows_with_the_chunk_count_not_with_the_matrix():
    from alpro_amd import hip
    lib = hip.load()
    # min(k, chunk) keys of 8 bytes per (query, chunk), 256-byte granules; a forced chunk is taken as given
    assert lib.alpro_sim_topk_workspace_bytes(3, 5000, 128, 32) == (3 * 157 * 32 * 8 + 255) // 256 * 256
    assert lib.alpro_sim_topk_workspace_bytes(33, 257, 10, 64) == (33 * 5 * 10 * 8 + 255) // 256 * 256
    # more than 2048 lists per query: a second level of k keys per (query, group of 2048 lists) behind the first
    lists = (100000 + 31) // 32
    assert lib.alpro_sim_topk_workspace_bytes(1, 100000, 16, 32) == (lists * 16 * 8 + 255) // 256 * 256 + 2 * 16 * 8
    big = lib.alpro_sim_topk_workspace_bytes(1000, 100000, 16, 0)
    assert 0 < big < 1000 * 100000 * 4 // 8        # under an eighth of the fp32 matrix it replaces


def test_wrapper_refuses_cpu_wrong_dtype_and_strided_inputs():
    from alpro_amd import hip
    q, g = torch.zeros(4, 256), torch.zeros(9, 256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.sim_topk(q, g, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.sim_topk(np.zeros((4, 256), dtype=np.float32), g, 3)


@pytest.mark.parametrize("kind", tc.KINDS)
def test_exact_case_builders_hold_what_they_claim(kind):
    grid = {np.float32(v * 2.0 ** -4) for v in (-1, 0, 1)}
    for nq, ng, k in tc.SHAPES:
        c = tc.exact_case(kind, nq, ng, k)
        assert c.q.shape == (nq, 256) and c.g.shape == (ng, 256) and c.q.dtype == c.g.dtype == np.float32
        assert set(np.unique(c.q)) <= grid and set(np.unique(c.g)) <= grid
        # exact in fp32: the fp32 product in numpy's order, and in reversed k order, equals the fp64 one bit for bit
        assert np.array_equal((c.q @ c.g.T).astype(np.float64), c.s64)
        assert np.array_equal((c.q[:, ::-1] @ c.g[:, ::-1].T).astype(np.float64), c.s64)
        assert np.abs(c.s64 * 256).max() <= 256 and np.array_equal(c.s64 * 256, np.round(c.s64 * 256))
        # the expectation is the stable descending sort: values never rise, equal values keep ascending indices, the tail is -1 / -inf
        n = min(k, ng)
        assert c.val.shape == c.idx.shape == (nq, k) and c.val.dtype == np.float32 and c.idx.dtype == np.int32
        assert (c.idx[:, n:] == -1).all() and np.isneginf(c.val[:, n:]).all()
        sv = np.take_along_axis(c.s64, c.idx[:, :n].astype(np.int64), axis=1)
        assert np.array_equal(c.val[:, :n], sv.astype(np.float32) * np.float32(c.scale))
        assert ((sv[:, :-1] > sv[:, 1:]) | ((sv[:, :-1] == sv[:, 1:]) & (c.idx[:, :n - 1] < c.idx[:, 1:n]))).all()
        for i in range(nq):   # nothing better left out, and of the candidates tied with the last one the smallest indices were taken
            rest = np.setdiff1d(np.arange(ng), c.idx[i, :n])
            if rest.size:
                assert c.s64[i, rest].max() <= sv[i, -1]
                tied = rest[c.s64[i, rest] == sv[i, -1]]
                assert tied.size == 0 or tied.min() > c.idx[i, :n][sv[i] == sv[i, -1]].max()
        if kind == "dup" and ng >= 6:
            m = ng // 3
            assert np.array_equal(c.g[:m], c.g[m:2 * m]) and np.array_equal(c.g[:m], c.g[2 * m:3 * m])
        if kind == "equal":
            assert (c.g == c.g[0]).all() and np.array_equal(c.idx[:, :n], np.tile(np.arange(n, dtype=np.int32), (nq, 1)))
        if kind == "edge_ties":
            edges = [e for e in tc.EDGES if e < ng]
            for e in edges:
                assert np.array_equal(c.g[e - 1], c.g[e])
            if edges:   # query 0's best candidates are exactly the edge rows, in index order: ties on both sides of every chunk edge
                want = sorted(j for e in edges for j in (e - 1, e))[:n]
                assert c.idx[0, :len(want)].tolist() == want and len(set(c.val[0, :len(want)].tolist())) == 1


def test_random_case_bound_is_far_above_the_fp32_error():
    c = tc.random_case(67, 1000, 32)
    assert np.allclose(np.linalg.norm(c.q, axis=1), 1, atol=1e-6) and np.allclose(np.linalg.norm(c.g, axis=1), 1, atol=1e-6)
    err = np.abs((c.q @ c.g.T).astype(np.float64) - c.s64).max()
    assert err < 1e-6 < c.bound.max() < 1e-4
    # check_random accepts the fp64 answer itself and refuses a swapped pair, a repeated index and a missing best candidate
    val, idx = tc.expected_topk(c.s64, c.k, 1.0)
    tc.check_random(c, val, idx)
    for breaker in ("swap", "repeat", "miss"):
        v, i = val.copy(), idx.copy()
        if breaker == "swap":
            v[0, [0, 1]], i[0, [0, 1]] = v[0, [1, 0]], i[0, [1, 0]]
        elif breaker == "repeat":
            v[0, 1], i[0, 1] = v[0, 0], i[0, 0]
        else:
            order = np.argsort(-c.s64[0], kind="stable")
            v[0, :-1], i[0, :-1] = v[0, 1:], i[0, 1:]
            v[0, -1], i[0, -1] = np.float32(c.s64[0, order[c.k]]), order[c.k]
        with pytest.raises(AssertionError):
            tc.check_random(c, v, i)


def _full_candidates(table):
    """every column a candidate, in column order, with the constant sim the reference's synthetic records carry"""
    n = table.shape[1]
    return torch.arange(n).repeat(table.shape[0], 1), torch.from_numpy(np.ascontiguousarray(table)), torch.zeros(table.shape, dtype=torch.float64)


def test_rerank_metrics_equal_the_reference_metrics_on_the_synthetic_table():
    from alpro_amd.retrieval_eval import rerank_metrics
    g = np.load(os.path.join(GOLDEN, "retrieval_eval_T2_V5.npz"))
    table = g["synthetic_table"]    # stored video-major, table[video, caption], like score_all_pairs' matrices (tests/golden/make_golden.py)
    for d, t in (("text2video", table.T), ("video2text", table)):    # so a caption's candidates are a column, a video's a row
        idx, score, sim = _full_candidates(t)
        m = rerank_metrics(idx, score, sim, torch.arange(12))
        assert m["outside"] == 0
        for key in ("r1", "r5", "r10", "medianR", "meanR"):
            assert m[key] == float(g["synthetic/%s/%s" % (d, key)]), (d, key, m[key])


def test_rerank_metrics_with_ten_of_twelve_candidates():
    from alpro_amd.retrieval_eval import rerank_metrics
    table = np.load(os.path.join(GOLDEN, "retrieval_eval_T2_V5.npz"))["synthetic_table"]
    for d, t in (("text2video", table.T), ("video2text", table)):
        # stage 1 orders by sim = the table itself (value descending, index ascending: what alpro_sim_topk returns) and keeps 10 of 12, so the
        # two candidates it drops rank below the other ten in the final order as well
        t = np.ascontiguousarray(t)
        order = np.argsort(-t, axis=1, kind="stable")
        i10 = torch.from_numpy(order[:, :10].copy())
        score = torch.from_numpy(t)
        gt = torch.arange(12)
        full = rerank_metrics(torch.arange(12).repeat(12, 1), score, score, gt)
        m = rerank_metrics(i10, score.gather(1, i10), score.gather(1, i10), gt)
        for key in ("r1", "r5", "r10"):
            assert m[key] == full[key], (d, key)
        sim_rank = 1 + np.argmax(order == np.arange(12)[:, None], axis=1)
        assert m["outside"] == int((sim_rank > 10).sum()) and full["outside"] == 0, d
        assert m["medianR"] <= full["medianR"] and m["meanR"] <= full["meanR"]       # an outside query counts as rank 11: lower bounds
        with pytest.raises(ValueError, match="k=9"):
            rerank_metrics(i10[:, :9], score.gather(1, i10)[:, :9], score.gather(1, i10)[:, :9], gt)
