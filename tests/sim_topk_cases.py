"""Cases for alpro_sim_topk (similarity + top-k without the matrix).  Shared by tests/test_sim_topk_gpu.py (GPU) and tests/test_sim_topk_cpu.py
(CPU self-check of the builders); not collected itself, numpy on the CPU only.

Exact cases: every feature is one of {-1, 0, 1} * 2^-4, so a product is one of {-1, 0, 1} * 2^-8 and every partial sum of the 256-term chain
is a multiple of 2^-8 of magnitude <= 1 -- exact in fp32 whatever the order.  The similarities are therefore known bit for bit (fp64 holds
them exactly), they tie all the time (513 possible values), and the expected (val, idx) is the fp64 matrix under a STABLE descending sort:
value descending, gallery index ascending.  out_val = fp32(s) * fp32(scale) is one correctly rounded fp32 multiply, which numpy reproduces.

Random cases: seeded unit-norm fp32 rows, the model's kind of feature.  The kernel's value may differ from fp64 by the worst case of a
256-term fp32 chain, B_ij = 256 * 2^-24 * sum_k |q_ik g_jk|; random_case returns the fp64 matrix and B for the checks of the GPU test.
"""
import zlib
from collections import namedtuple

import numpy as np

D = 256
SHAPES = ((1, 1, 1), (1, 31, 10), (33, 257, 10), (67, 1000, 32), (3, 5000, 128), (5, 5, 10))   # (nq, ng, k); the last has ng < k
CHUNKS = (0, 32, 64)          # 0 = the library's choice; ng = 257 with chunk 64 leaves one row in the last chunk
KINDS = ("random", "dup", "equal", "edge_ties")
EDGES = (32, 64, 128, 256, 512)   # chunk edges of CHUNKS and of every default the library may pick (128 .. 512 rows)
SCALE = float(np.float32(1.0) / np.float32(0.07))   # 1 / temp of the model: not a power of two, so the one multiply rounds

ExactCase = namedtuple("ExactCase", "name q g k scale val idx s64")
RandomCase = namedtuple("RandomCase", "name q g k s64 bound")


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7fffffff)


def _trits(rng, rows):
    return (rng.randint(-1, 2, size=(rows, D)).astype(np.float32) * np.float32(2.0 ** -4))


def expected_topk(s64, k, scale):
    """(val (nq, k) fp32, idx (nq, k) int32) of an exactly known similarity matrix: stable descending sort, -inf / -1 behind ng."""
    nq, ng = s64.shape
    s = s64 + 0.0                                              # -0.0 -> +0.0
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]       # ties keep the ascending index
    val = np.full((nq, k), -np.inf, dtype=np.float32)
    idx = np.full((nq, k), -1, dtype=np.int32)
    n = min(k, ng)
    idx[:, :n] = order[:, :n]
    val[:, :n] = np.take_along_axis(s, order[:, :n], axis=1).astype(np.float32) * np.float32(scale)
    return val, idx


def exact_case(kind, nq, ng, k):
    rng = _rng("exact", kind, nq, ng, k)
    q = _trits(rng, nq)
    if kind == "random":
        g = _trits(rng, ng)
    elif kind == "dup":                    # every gallery row occurs several times, far apart: g[j] = g[j % m]
        m = max(1, ng // 3)
        g = _trits(rng, m)[np.arange(ng) % m]
    elif kind == "equal":                  # one row, ng times: every query ties over the whole gallery
        g = np.repeat(_trits(rng, 1), ng, axis=0)
    elif kind == "edge_ties":              # the rows on both sides of every chunk edge are the same row, and query 0's best match
        g = _trits(rng, ng)
        hot = np.where(q[0] == 0, np.float32(2.0 ** -4), q[0])
        for e in EDGES:
            if e < ng:
                g[e - 1] = hot
                g[e] = hot
    else:
        raise ValueError(kind)
    q, g = np.ascontiguousarray(q), np.ascontiguousarray(g)
    s64 = q.astype(np.float64) @ g.astype(np.float64).T
    val, idx = expected_topk(s64, k, SCALE)
    return ExactCase("%s_q%d_g%d_k%d" % (kind, nq, ng, k), q, g, k, SCALE, val, idx, s64)


def random_case(nq, ng, k):
    rng = _rng("unit", nq, ng, k)
    q = rng.standard_normal((nq, D)).astype(np.float32)
    g = rng.standard_normal((ng, D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True).astype(np.float32)
    q, g = np.ascontiguousarray(q), np.ascontiguousarray(g)
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    s64 = q64 @ g64.T
    bound = 256.0 * 2.0 ** -24 * (np.abs(q64) @ np.abs(g64).T)
    return RandomCase("unit_q%d_g%d_k%d" % (nq, ng, k), q, g, k, s64, bound)


def check_random(case, val, idx):
    """The four properties of a correct result on inexact data (val, idx: numpy arrays from the kernel, scale = 1).  Raises AssertionError."""
    nq, ng = case.s64.shape
    k = case.k
    n = min(k, ng)
    assert val.shape == (nq, k) and idx.shape == (nq, k)
    assert (idx[:, n:] == -1).all() and np.isneginf(val[:, n:]).all(), "tail behind ng"
    vi, ii = val[:, :n].astype(np.float64), idx[:, :n].astype(np.int64)
    assert ((ii >= 0) & (ii < ng)).all(), "index range"
    ref = np.take_along_axis(case.s64, ii, axis=1)
    err = np.abs(vi - ref)
    lim = np.take_along_axis(case.bound, ii, axis=1)
    print("%s: max |val - fp64| %.3e (max bound %.3e)" % (case.name, err.max(), case.bound.max()))
    assert (err <= lim).all(), "value error %.3e above the chain bound" % (err - lim).max()
    ordered = (val[:, :n - 1] > val[:, 1:n]) | ((val[:, :n - 1] == val[:, 1:n]) & (idx[:, :n - 1] < idx[:, 1:n]))
    assert ordered.all(), "rows must be sorted by (val desc, idx asc)"
    assert all(len(set(row.tolist())) == n for row in ii), "an index returned twice"
    taken = np.zeros((nq, ng), dtype=bool)
    np.put_along_axis(taken, ii, True, axis=1)
    floor = ref.min(axis=1, keepdims=True) + 2.0 * case.bound.max()
    left = np.where(taken, -np.inf, case.s64)
    assert (left <= floor).all(), "a better candidate was left out by %.3e" % (left - floor).max()
