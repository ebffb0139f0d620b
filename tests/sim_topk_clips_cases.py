"""Cases for alpro_sim_topk_clips (top-k by pooled similarity, several clips per video).  They extend tests/sim_topk_cases.py; shared by
tests/test_vr_clips_sim_topk_gpu.py (GPU) and tests/test_sim_topk_clips_cpu.py (CPU self-check); not collected itself, numpy on the CPU only.

A case has `lists` result rows over `ent` gallery entries and n clips on one side:
    GALLERY (text -> video): q (lists, 256), g (ent * n, 256) with row e * n + j; the entries are videos.
    QUERY   (video -> text): q (lists * n, 256) with row v * n + j, g (ent, 256); the entries are rows of g.
Everything is expressed on the cube x[list, entry, j], the value of clip j.

Exact cases: features in {-1, 0, 1} * 2^-4 make every s_j exact (sim_topk_cases); x_j = fp32(s_j) * fp32(SCALE) is one numpy fp32 multiply;
mean = numpy fp32 sequential adds from 0 in ascending j, then / np.float32(n) (a correctly rounded division, as the library's); max is exact.
So mean and max are known BIT FOR BIT, and the expectation is the stable descending sort of the pooled fp32 matrix (-0.0 read as +0.0).
lse goes through expf / logf and is checked by properties against fp64, like the random (unit-norm) cases of every mode.

Error bound of a pooled value against fp64 (pool64 of s64 * scale), first order, DERIVED, not measured.  All three pools are 1-Lipschitz in the
sup norm, so the error of the inputs passes through at most once:
    input part    |scale| * max_j B_j + 2^-24 * X      B_j = the 256-term chain bound of sim_topk_cases (0 on exact cases), X = max_j |x_j|;
                                                       the second term is the rounding of the one multiply by scale.
    mean          2^-24 * n * X                         n - 1 adds, each rounding a partial sum of magnitude <= n X, i.e. (n - 1) 2^-24 X after
                                                       the division by n, plus the division's own rounding 2^-24 X.
    max           0
    lse           2^-24 * (2 X + n + 4 ln n + 4 + |P|)  with S = sum_j exp(x_j - m) in [1, n], P = m + log S, and expf / logf within 2 ulp:
                                                       x_j - m rounds by 2^-24 |x_j - m| <= 2^-24 * 2 X, a relative error of each term and so
                                                       of S, i.e. an absolute error of log S             -> 2 X
                                                       expf: 2 ulp = 4 * 2^-24 relative on every term    -> 4
                                                       the n - 1 adds of the sum, 2^-24 relative each    -> n
                                                       logf: 2 ulp of log S <= ln n                      -> 4 ln n
                                                       the final add m + log S rounds by 2^-24 |P|       -> |P|
"""
from collections import namedtuple

import numpy as np

from tests.sim_topk_cases import CHUNKS, D, KINDS, SCALE, _rng, _trits   # noqa: F401 (CHUNKS and KINDS are the tests')

GALLERY, QUERY = "gallery", "query"
MODES = ("mean", "max", "lse")
# GALLERY (nq, nvid, n, k): 258 gallery rows with n not dividing 32; n at the cap with nvid < k; many query tiles; several sub-passes of 73 videos
GALLERY_SHAPES = ((1, 1, 1, 1), (1, 1, 3, 1), (33, 86, 3, 10), (5, 5, 32, 10), (67, 1000, 2, 32), (3, 700, 7, 128))
# QUERY (nvid, n, ng, k): 33 query rows in tiles of 10 videos; one video per tile; a long gallery; ng < k
QUERY_SHAPES = ((1, 1, 1, 1), (1, 3, 31, 10), (11, 3, 257, 10), (3, 32, 1000, 32), (2, 5, 5000, 128), (5, 7, 5, 10))
EPS = 2.0 ** -24

ClipCase = namedtuple("ClipCase", "name side q g lists ent n k scale s64 x64 chain")   # cubes (lists, ent, n): s64, x64 = s64 * scale, chain = |scale| * B


def shapes(side):
    """(lists, ent, n, k) of every shape of a side"""
    return [(nq, nvid, n, k) for nq, nvid, n, k in GALLERY_SHAPES] if side == GALLERY else [(nvid, ng, n, k) for nvid, n, ng, k in QUERY_SHAPES]


def edges(side, n):
    """gallery entries at which a chunk or a sub-pass may end: the chunk edges of sim_topk_cases, and for GALLERY the floor(512 / n) videos of a sub-pass"""
    e = {32, 64, 128, 256, 512}
    if side == GALLERY:
        e.add(512 // n)
    return sorted(e)


def _cube(side, s, lists, ent, n):
    return s.reshape(lists, ent, n) if side == GALLERY else np.ascontiguousarray(s.reshape(lists, n, ent).transpose(0, 2, 1))


def _case(name, side, q, g, lists, ent, n, k, scale, with_chain):
    q, g = np.ascontiguousarray(q), np.ascontiguousarray(g)
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    s64 = _cube(side, q64 @ g64.T, lists, ent, n)
    chain = _cube(side, 256.0 * EPS * (np.abs(q64) @ np.abs(g64).T), lists, ent, n) * abs(float(scale)) if with_chain else np.zeros_like(s64)
    return ClipCase(name, side, q, g, lists, ent, n, k, float(scale), s64, s64 * float(scale), chain)


def exact_case(side, kind, lists, ent, n, k):
    """trit features; `kind` shapes the gallery ENTRIES as in sim_topk_cases (a video entry keeps n different clips)"""
    rng = _rng("exact_clips", side, kind, lists, ent, n, k)
    per_ent = n if side == GALLERY else 1                  # rows of g per entry
    q = _trits(rng, lists * (1 if side == GALLERY else n))
    if kind == "random":
        g = _trits(rng, ent * per_ent)
    elif kind == "dup":                                    # every entry occurs several times, far apart
        m = max(1, ent // 3)
        g = _trits(rng, m * per_ent).reshape(m, per_ent, D)[np.arange(ent) % m].reshape(ent * per_ent, D)
    elif kind == "equal":                                  # one entry, ent times: every list ties over the whole gallery
        g = np.tile(_trits(rng, per_ent), (ent, 1))
    elif kind == "edge_ties":                              # the entries on both sides of every edge are the same, and list 0's best match
        g = _trits(rng, ent * per_ent)
        if side == QUERY:
            q[:n] = q[0]                                   # video 0: n equal clips, so `hot` is the best row for every clip and every pool
        hot = np.where(q[0] == 0, np.float32(2.0 ** -4), q[0])
        for e in edges(side, n):
            if e < ent:
                g[(e - 1) * per_ent:(e + 1) * per_ent] = hot
    else:
        raise ValueError(kind)
    return _case("%s_%s_l%d_e%d_n%d_k%d" % (side, kind, lists, ent, n, k), side, q, g, lists, ent, n, k, SCALE, False)


def random_case(side, lists, ent, n, k):
    """seeded unit-norm fp32 rows, the model's kind of feature, scale = 1 / temp"""
    rng = _rng("unit_clips", side, lists, ent, n, k)
    q = rng.standard_normal((lists * (1 if side == GALLERY else n), D)).astype(np.float32)
    g = rng.standard_normal((ent * (n if side == GALLERY else 1), D)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True).astype(np.float32)
    return _case("%s_unit_l%d_e%d_n%d_k%d" % (side, lists, ent, n, k), side, q, g, lists, ent, n, k, SCALE, True)


def pool32(case, mode):
    """the pooled (lists, ent) fp32 matrix of an EXACT case, bit for bit, for mean and max"""
    assert mode in ("mean", "max") and not case.chain.any()
    x = case.s64.astype(np.float32) * np.float32(case.scale)     # s is exact in fp32; one fp32 multiply
    if mode == "max":
        return x.max(axis=2)
    s = np.zeros(x.shape[:2], dtype=np.float32)
    for j in range(case.n):
        s = s + x[:, :, j]
    return s / np.float32(case.n)


def pool64(case, mode):
    """the pooled (lists, ent) matrix in fp64"""
    x = case.x64
    if mode == "mean":
        return x.mean(axis=2)
    m = x.max(axis=2)
    return m if mode == "max" else m + np.log(np.exp(x - m[:, :, None]).sum(axis=2))


def bound(case, mode):
    """(lists, ent) bound of |kernel value - pool64| (module docstring)"""
    X = np.abs(case.x64).max(axis=2)
    b = case.chain.max(axis=2) + EPS * X
    if mode == "mean":
        b = b + EPS * case.n * X
    elif mode == "lse":
        b = b + EPS * (2 * X + case.n + 4 * np.log(case.n) + 4 + np.abs(pool64(case, mode)))
    return b


def expected_topk(p32, k):
    """(val (lists, k) fp32, idx (lists, k) int32) of a pooled fp32 matrix known bit for bit: stable descending sort, -inf / -1 behind the gallery"""
    lists, ent = p32.shape
    p = p32 + np.float32(0.0)                                  # -0.0 -> +0.0
    order = np.argsort(-p.astype(np.float64), axis=1, kind="stable")[:, :k]
    val = np.full((lists, k), -np.inf, dtype=np.float32)
    idx = np.full((lists, k), -1, dtype=np.int32)
    m = min(k, ent)
    idx[:, :m] = order[:, :m]
    val[:, :m] = np.take_along_axis(p, order[:, :m], axis=1)
    return val, idx


def check_pooled(case, mode, val, idx):
    """The four properties of a correct result on inexact values (sim_topk_cases.check_random on the pooled matrix).  Raises AssertionError."""
    lists, ent, k = case.lists, case.ent, case.k
    m = min(k, ent)
    p64, lim_all = pool64(case, mode), bound(case, mode)
    assert val.shape == (lists, k) and idx.shape == (lists, k)
    assert (idx[:, m:] == -1).all() and np.isneginf(val[:, m:]).all(), "tail behind the gallery"
    vi, ii = val[:, :m].astype(np.float64), idx[:, :m].astype(np.int64)
    assert ((ii >= 0) & (ii < ent)).all(), "index range"
    ref = np.take_along_axis(p64, ii, axis=1)
    err = np.abs(vi - ref)
    lim = np.take_along_axis(lim_all, ii, axis=1)
    print("%s %s: max |val - fp64| %.3e (bound there %.3e, max bound %.3e)" % (case.name, mode, err.max(), lim.reshape(-1)[err.argmax()], lim_all.max()))
    assert (err <= lim).all(), "value error above the bound by %.3e" % (err - lim).max()
    ordered = (val[:, :m - 1] > val[:, 1:m]) | ((val[:, :m - 1] == val[:, 1:m]) & (idx[:, :m - 1] < idx[:, 1:m]))
    assert ordered.all(), "rows must be sorted by (val desc, idx asc)"
    assert all(len(set(row.tolist())) == m for row in ii), "an index returned twice"
    taken = np.zeros((lists, ent), dtype=bool)
    np.put_along_axis(taken, ii, True, axis=1)
    floor = ref.min(axis=1, keepdims=True) + 2.0 * lim_all.max()
    left = np.where(taken, -np.inf, p64)
    assert (left <= floor).all(), "a better candidate was left out by %.3e" % (left - floor).max()

