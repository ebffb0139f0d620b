"""Cases, references and order emulators for the kernels that only MOVE rows: alpro_transpose / _transpose_batch, alpro_gather_cast, the
three forms of alpro_scatter_add_rows (ordered indexed, position, atomic), alpro_gather_seq_fwd / _bwd, alpro_patchify, alpro_cls_mean_bwd
and (the one inexact kernel of the group) alpro_gelu_bwd.  Shared by tests/test_hip_movement_exact.py (GPU) and
tests/test_movement_cases_cpu.py (CPU self-check); not collected itself, torch on the CPU only.

Exact inputs.  These kernels copy, scale a row by one factor, cast and add.  Values are integers with |x| <= 64 (or those times a power of
two), row scales and cls_scale are powers of two, dropout runs at p = 0.5 (keep scale 2), and every sum stays below 2^24 in units of its
finest term: any fp32 summation order then gives the bits of the int64 / fp64 reference, and a 16-bit output holds the value itself.
fp32-to-fp32 copies carry row-identifying data (row * 1024 + col), so a wrong row or column shows as such.

Order-sensitive inputs.  The ordered indexed scatter, the position scatter and gather_seq_bwd promise ascending source order into an
accumulator that starts at 0 (d32[s] before d_t[s] within one s for gather_seq_bwd); the scatters then add the total to the destination's
previous content in ONE fp32 add.  A tolerance cannot see an order, so these run on fp32 values with a wide exponent spread
(randn * 2^randint(-12, 12)) against emulate_runs, which performs exactly those fp32 additions on the CPU (additions only: no FMA
contraction to worry about).  tests/test_movement_cases_cpu.py checks that the inputs do tell ascending from descending and random order.

References are written from the layouts, not from the kernels: token rows (b, 1 + n*T + t) and frame rows ((b*T + t), 1 + n) for the
three row maps, index_add_ in fp64 for the scatters, torch.cat([text[ti], video[vi]], 1) and its autograd for gather_seq, F.unfold for
patchify.  Outputs and destinations sit inside SENTINEL-filled buffers, sources inside NaN-filled ones (tests/gemm_cases.py poisoned).
"""
import functools
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests.gemm_cases import (_BUILT, BF16, DT_NAME, F16, F32, F64, MAP_FRAME_TOKENS, MAP_IDENTITY, MAP_PATCH_EMBED, MAP_SKIP_CLS, SENTINEL, Inputs, gen, ints,
                              keep_mask, lossless, poisoned)

D = 768
GUARD = 4                 # guard rows before / behind every output view
LIMIT = 2.0 ** 24
DROP_P = 0.5
DTS = (F32, BF16, F16)
MAP_NAME = {MAP_IDENTITY: "identity", MAP_SKIP_CLS: "skip_cls", MAP_FRAME_TOKENS: "frame", MAP_PATCH_EMBED: "patch"}


def same(got, want):
    """THE comparison of the exact and the order cases: every element of a buffer (guards included), zero tolerance.  `want` is moved to
    got's device, so the large tables are compared where they lie."""
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.detach(), want.to(got.device))


def first_mismatch(got, want):
    """(row, column, got, want) of the first differing element of two 2-D buffers, for the failure message."""
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    bad = ((g != w) | g.isnan()).nonzero()
    if bad.numel() == 0:
        return None
    r, c = int(bad[0, 0]), int(bad[0, 1])
    return r, c, float(g[r, c]), float(w[r, c])


def row_ident(R, C, row0=0):
    """value = row * 1024 + col (row * 4096 + col for rows wider than 1024): exact in fp32, every element of a matrix names its place."""
    stride = 1024 if C <= 1024 else 4096
    v = torch.arange(row0, row0 + R)[:, None] * stride + torch.arange(C)[None, :]
    assert int(v.max()) < LIMIT
    return v.to(F64)


def wide(shape, g):
    """Order-sensitive fp32 data: randn * 2^randint(-12, 12) per element."""
    return torch.randn(shape, generator=g) * torch.exp2(torch.randint(-12, 13, shape, generator=g).float())


def pow2_scales(n, g):
    """Row scales from {0.5, 1, 2, 4}, neighbours different."""
    v = torch.randint(0, 4, (n,), generator=g)
    for i in range(1, n):
        if v[i] == v[i - 1]:
            v[i] = (v[i] + 1) % 4
    return torch.exp2(v.float() - 1.0)


# ------------------------------------------------------------------------------------------------ fp32 sums in a stated order
def seq_sum(terms):
    """(k, ...) fp32 -> the sum of the k rows taken one after the other from 0, one fp32 add each (numpy's accumulate keeps the element
    type and the order; torch's CPU cumsum and sum accumulate in fp64 or pairwise)."""
    import numpy as np
    a = terms.contiguous().numpy().reshape(terms.shape[0], -1)
    return torch.from_numpy(np.add.accumulate(a, axis=0, dtype=np.float32)[-1].copy()).view(terms.shape[1:])


RUN_LONG = 64


def emulate_runs(src, dest, n_dest, order="asc", g=None):
    """acc[d] = the fp32 sum, from 0, of the rows src[i] with dest[i] == d, taken in ascending i ("asc": the documented order), descending i
    ("desc") or a random order ("random", generator g).  src (n, ...) fp32, dest (n,) int64 in [0, n_dest).  One fp32 add per term: long
    runs one destination at a time (seq_sum), the short ones rank by rank, the k-th term of every destination at once."""
    assert src.dtype == F32
    n = dest.numel()
    acc = torch.zeros((n_dest,) + tuple(src.shape[1:]), dtype=F32)
    if n == 0:
        return acc
    pos = torch.arange(n)
    key = pos if order == "asc" else n - 1 - pos if order == "desc" else torch.randperm(n, generator=g)
    by_key = torch.argsort(key)                                        # the sources in the order they are to be taken
    grouped = by_key[torch.argsort(dest[by_key], stable=True)]         # ... grouped by destination, that order kept inside a group
    counts = torch.bincount(dest, minlength=n_dest)
    starts = torch.cumsum(counts, 0) - counts
    for d in (counts >= RUN_LONG).nonzero().view(-1).tolist():
        acc[d] = seq_sum(src[grouped[starts[d]:starts[d] + counts[d]]])
    short = counts[dest[grouped]] < RUN_LONG
    if not bool(short.any()):
        return acc
    rank = (torch.arange(n) - starts[dest[grouped]])[short]            # position of each source inside its destination's sequence
    grouped = grouped[short]
    by_rank = torch.argsort(rank, stable=True)
    lo = 0
    for hi in torch.cumsum(torch.bincount(rank), 0).tolist():
        i = grouped[by_rank[lo:hi]]
        acc[dest[i]] = acc[dest[i]] + src[i]
        lo = hi
    return acc


# ------------------------------------------------------------------------------------------------ transpose
TR_R, TR_C, TR_PADS = (1, 63, 64, 65, 129), (1, 63, 64, 65, 200), (64, 128, 256)
TR_DTYPES = ((F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16))
TR_GUARD_COLS = 8
TrCase = namedtuple("TrCase", "R C pad_to din dout strided")
TRANSPOSE_CASES = tuple(TrCase(R, C, p, din, dout, s) for (din, dout) in TR_DTYPES for p in TR_PADS for R in TR_R for C in TR_C for s in (False, True))


def tr_id(c):
    return "%dx%d-pad%d-%s_%s%s" % (c.R, c.C, c.pad_to, DT_NAME[c.din], DT_NAME[c.dout], "-strided" if c.strided else "")


def rpad(R, pad_to):
    return (R + pad_to - 1) // pad_to * pad_to


def matrix(R, C, din, dout, *key):
    """(R, C) fp64 source of a transpose: row-identifying for the fp32 copy, integers in [-64, 64] where a 16-bit type is involved."""
    if din == F32 and dout == F32:
        return row_ident(R, C)
    return ints((R, C), gen("matrix", R, C, *key), -64, 64)


def transpose_inputs(c):
    """-> dict(x (R, C) fp64, colsum0 (C,) fp32 non-zero integers, colsum (C,) fp64 = colsum0 + column sums)."""
    x = matrix(c.R, c.C, c.din, c.dout, c.pad_to)
    cs0 = ints((c.C,), gen("tr_cs", c.R, c.C), 1, 100)
    return dict(x=x, colsum0=cs0.to(F32), colsum=cs0 + x.sum(0))


def transpose_ref(x64, Rpad):
    """out[c, r] = x[r, c] for r < R, +0 for R <= r < Rpad."""
    R, C = x64.shape
    out = torch.zeros(C, Rpad, dtype=F64)
    for r in range(R):
        out[:, r] = x64[r]
    return out


def transpose_expected(x64, Rpad, dout, guard_cols=TR_GUARD_COLS, fault=None):
    """The CPU image of the whole output buffer: (GUARD + C + GUARD, Rpad + guard_cols), SENTINEL outside the (C, Rpad) view at row GUARD."""
    ref = transpose_ref(x64, Rpad)
    R = x64.shape[0]
    if fault == "unzeroed_pad_column" and Rpad > R:
        ref[:, Rpad - 1] = SENTINEL
    buf = poisoned(ref.to(dout), GUARD, guard_cols, GUARD, fill=SENTINEL)._base
    if fault == "guard_overwritten":
        buf[GUARD + x64.shape[1], 0] = 0.0
    return buf


def pad_is_plus_zero(buf, C, R, Rpad):
    """The pad columns R <= r < Rpad of the view hold +0, not -0 (torch.equal cannot tell)."""
    pad = buf.detach().cpu()[GUARD:GUARD + C, R:Rpad].float()
    return bool((pad == 0).all()) and not bool(torch.signbit(pad).any())


# transpose_batch job tables: (R, C, extra columns of Rpad beyond R rounded to 64).  The mixed table puts a one-tile job first, last and
# between the two large ones.
TB_MIXED = ((1, 1, 0), (768, 3072, 0), (64, 64, 64), (3072, 768, 128), (65, 63, 0), (200, 300, 64), (1, 1, 192))
TB_TABLES = {"one": ((65, 63, 64),), "mixed": TB_MIXED,
             "many": tuple((1 + (37 * j) % 130, 1 + (53 * j) % 150, 64 * (j % 3)) for j in range(130))}


# ------------------------------------------------------------------------------------------------ gather_cast
GC_DIMS = ((1, 1, 1), (2, 4, 9), (3, 8, 5), (1, 128, 2))
GC_IDENTITY_ROWS = (1, 2, 7, 8191)
GC_COLSUMS = ("none", "colsum", "pre", "both")
GC_CLS_SCALE = 2.0 ** -3
GcCase = namedtuple("GcCase", "mode dims rows dt group drop colsum det")


def gc_id(c):
    return "%s-%s-%s-g%d-%s-%s-%s" % (MAP_NAME[c.mode], "r%d" % c.rows if c.dims is None else "b%dt%dn%d" % c.dims, DT_NAME[c.dt], c.group, "drop" if c.drop else "nodrop",
                                      c.colsum, "det" if c.det else "atomic")


def gc_rows(mode, dims):
    B, T, N = dims
    return {MAP_SKIP_CLS: B * N * T, MAP_FRAME_TOKENS: B * T * (N + 1), MAP_PATCH_EMBED: B * T * N}[mode]


def gc_groups(mode, dims, rows):
    """Row-scale groups of a shape: none (0), 1, T, N + 1, S and one that divides neither the rows per clip nor the row count."""
    B, T, N = dims if dims is not None else (1, 2, 2)
    per_clip = rows // B
    odd = next(g for g in (5, 7, 11, 13, 17) if per_clip % g and rows % g or rows < g)
    return tuple(dict.fromkeys((0, 1, T, N + 1, 1 + N * T, odd)))


def _build_gc_cases():
    cs = []
    for mode in (MAP_IDENTITY, MAP_SKIP_CLS, MAP_FRAME_TOKENS, MAP_PATCH_EMBED):
        shapes = [(None, r) for r in GC_IDENTITY_ROWS] if mode == MAP_IDENTITY else [(d, gc_rows(mode, d)) for d in GC_DIMS]
        for dt in DTS:
            k = 0
            for dims, rows in shapes:
                for group in gc_groups(mode, dims, rows):
                    for drop in (False, True):
                        # the eight (colsum, mode) settings in turn: each shape sees all of them, each group and dropout setting several
                        cs.append(GcCase(mode, dims, rows, dt, group, drop, GC_COLSUMS[k % 4], (k // 4) % 2 == 0))
                        k += 1
                k += 1      # (12 cases per shape: shift by one so that the next shape pairs the settings differently)
    return tuple(cs)


GATHER_CAST_CASES = _build_gc_cases()


def map_src_rows(mode, dims, rows):
    """-> (src (rows,) int64 token row each output row reads, is_cls (rows,) bool), from the layouts: a clip's tokens are row b*S of [CLS]
    and rows b*S + 1 + n*T + t of patch n, frame t (S = 1 + N*T); SKIP_CLS lists a clip's patch tokens in that order; the frame layout has
    row (b*T + t)*(N+1) for the frame's copy of [CLS] and rows (b*T + t)*(N+1) + 1 + n for its patches; PATCH_EMBED rows are (b*T + t)*N + n."""
    m = torch.arange(rows)
    if mode == MAP_IDENTITY:
        return m, torch.zeros(rows, dtype=torch.bool)
    B, T, N = dims
    S = 1 + N * T

    def token(b, n, t):
        return b * S + 1 + n * T + t
    if mode == MAP_SKIP_CLS:
        b, k = m // (N * T), m % (N * T)
        return token(b, k // T, k % T), torch.zeros(rows, dtype=torch.bool)
    width = N + 1 if mode == MAP_FRAME_TOKENS else N
    frame, j = m // width, m % width
    b, t = frame // T, frame % T
    if mode == MAP_PATCH_EMBED:
        return token(b, j, t), torch.zeros(rows, dtype=torch.bool)
    return torch.where(j == 0, b * S, token(b, (j - 1).clamp(min=0), t)), j == 0


@functools.lru_cache(maxsize=1)
def keep_rows(seed, rows):
    """(rows, 768) {0, 1}: the dropout mask of element row * 768 + col (tests/gemm_cases.py keep_mask; the cases of one shape follow each other)."""
    return keep_mask(seed, rows, D)


def gc_build(c):
    """Inputs of a gather_cast case (the same for the three output dtypes): integers in [-16, 16], scales from {0.5, 1, 2, 4}, cls_scale 2^-3."""
    key = ("gc",) + tuple(c._replace(dt=None, det=None, colsum=None))
    if key in _BUILT:
        return _BUILT[key]
    g = gen(*key)
    x = Inputs()
    B, T, N = c.dims if c.dims is not None else (1, 1, 1)
    x.src_rows = c.rows if c.mode == MAP_IDENTITY else B * (1 + N * T)
    x.src = ints((x.src_rows, D), g, -16, 16).to(F32)
    x.p0, x.p1 = {MAP_IDENTITY: (0, 0), MAP_SKIP_CLS: (N * T, 0), MAP_FRAME_TOKENS: (T, N), MAP_PATCH_EMBED: (T, N)}[c.mode]
    x.row_scale = pow2_scales((c.rows + c.group - 1) // c.group, g) if c.group else None
    x.cls_scale = GC_CLS_SCALE if c.mode == MAP_FRAME_TOKENS else 1.0
    x.drop_seed = 1 + zlib.crc32(repr(key).encode()) % 100000 if c.drop else 0
    x.colsum0, x.pre0 = ints((D,), g, 1, 100).to(F32), ints((D,), g, -100, -1).to(F32)
    x.ref = gc_reference(c, x)
    _BUILT[key] = x
    return x


def gc_reference(c, x, fault=None, f=F64, perm=None):
    """out[m] = row_scale[m // group] * (cls_scale on [CLS] rows) * dropout(src[row(m)]) -> dict(out (rows, 768), colsum = colsum0 + out.sum(0),
    pre = pre0 + the sum of the rows after dropout and before any scale, unit = the finest term's grid, total = sum of |terms|).
    fault "src_row_off_by_one": every row read one token row further on; f / perm: evaluate in fp32 with the rows summed one by one in
    another order (the CPU self-check)."""
    row, is_cls = map_src_rows(c.mode, c.dims, c.rows)
    if fault == "src_row_off_by_one":
        row = (row + 1).clamp(max=x.src_rows - 1)
    v = x.src.to(f)[row]
    if x.drop_seed:
        v = v * keep_rows(x.drop_seed, c.rows).to(f) / (1.0 - DROP_P)
    pre_terms = v
    sc = torch.ones(c.rows, dtype=f)
    if x.row_scale is not None:
        sc = x.row_scale.to(f)[torch.arange(c.rows) // c.group]
    sc = torch.where(is_cls, sc * x.cls_scale, sc)
    out = v * sc[:, None]
    order = perm if perm is not None else torch.arange(c.rows)
    unit = (min(float(sc.min()), 1.0))
    total = seq_sum if f == F32 else (lambda t: t.sum(0))
    return dict(out=out, colsum=x.colsum0.to(f) + total(out[order]), pre=x.pre0.to(f) + total(pre_terms[order]), unit=unit,
                total=max(float(out.abs().sum(0).max()), float(pre_terms.abs().sum(0).max())) + 100.0)


def gc_expected(c, x, fault=None):
    """The whole output buffer: (GUARD + rows + GUARD, 768) in c.dt."""
    ref = x.ref if fault != "src_row_off_by_one" else gc_reference(c, x, fault)
    out = ref["out"].to(c.dt)
    if fault == "last_row_dropped":
        out[c.rows - 1] = SENTINEL
    buf = poisoned(out, GUARD, 0, GUARD, fill=SENTINEL)._base
    if fault == "guard_overwritten":
        buf[GUARD + c.rows, 5] = 0.0
    return buf


# ------------------------------------------------------------------------------------------------ scatters
SC_ROWS, SC_TABLES, SC_TOP = (1, 2, 5, 4096, 8191, 8192), (1, 7, 30522), (1 << 19) - 1
SC_PATTERNS = ("equal", "perm", "mix", "top_last", "skip_min", "skip_max", "skip_only", "skip_absent", "oob")
SC_ORDER_PATTERNS = ("equal", "mix", "top_last", "skip_min", "oob")
ScCase = namedtuple("ScCase", "rows V pattern kind")       # kind: "exact" | "order"


def sc_id(c):
    return "%d-to-%d-%s-%s" % (c.rows, c.V, c.pattern, c.kind)


def _build_sc_cases():
    cs = []
    for rows in SC_ROWS:
        for V in SC_TABLES:
            for p in SC_PATTERNS:
                if p == "perm" and V < rows:
                    continue
                cs.append(ScCase(rows, V, p, "exact"))
                # an order case needs destinations with at least 3 terms: one row taking all of 5, or thousands of rows
                if p in SC_ORDER_PATTERNS and (rows >= 5 if p == "equal" else rows >= 4096 and V > 1):
                    cs.append(ScCase(rows, V, p, "order"))
    # the 19-bit key field's last value: only the first and the last table row are touched
    cs += [ScCase(8192, SC_TOP, "ends", "exact"), ScCase(8192, SC_TOP, "ends", "order")]
    return tuple(cs)


ORDERED_SCATTER_CASES = _build_sc_cases()
MOD_CASES = ((1, 1), (5, 7), (40, 40), (5120, 40), (130, 33), (7, 4), (9, 5))      # (rows, idx_mod) of the position form
MOD_TABLE_ROWS = 48
# The routes that do not range-check (in-range indices, exact inputs): route -> (reproducible mode, cases).  torch's index_put_ above 8192 rows;
# the atomic kernel with an index vector, without and with skip_idx; and idx None with skip_idx >= 0, (rows, idx_mod, skip_idx), which runs the
# atomic kernel in either mode.
OTHER_ROUTE_CASES = {
    "torch_8193": (True, (ScCase(8193, 7, "mix", "exact"), ScCase(8193, 30522, "top_last", "exact"))),
    "atomic_idx": (False, (ScCase(5, 7, "equal", "exact"), ScCase(4096, 30522, "perm", "exact"), ScCase(8193, 7, "top_last", "exact"))),
    "atomic_idx_skip": (False, (ScCase(4096, 7, "mix", "exact"), ScCase(8191, 30522, "skip_max", "exact"), ScCase(5, 7, "skip_only", "exact"))),
}
MOD_SKIP_CASES = ((130, 33, 3), (5120, 40, 0), (5, 7, 6), (7, 4, 3))
MOD_SKIP_ROUTES = {"atomic_mod_skip": False, "det_mod_skip": True}
OTHER_ROUTES = tuple(OTHER_ROUTE_CASES) + tuple(MOD_SKIP_ROUTES)


def sc_indices(rows, V, pattern, g):
    """-> (idx (rows,) int64, skip_idx)."""
    idx = torch.randint(0, V, (rows,), generator=g)
    skip = -1
    if pattern == "equal":
        idx[:] = V // 2
    elif pattern == "perm":
        idx = torch.randperm(V, generator=g)[:rows]
    elif pattern == "mix":                      # tests/test_hip_bwd_ops.py's token ids: [CLS] / [SEP] / [MASK] duplicates and a skipped pad row
        idx = torch.randint(min(4, V - 1), V, (rows,), generator=g)
        idx[::40] = 1 % V
        idx[7::40] = 2 % V
        idx[torch.rand(rows, generator=g) < 0.15] = 3 % V
        idx[torch.rand(rows, generator=g) < 0.2] = 0
        skip = 0
    elif pattern == "top_last":                 # the highest key: its run is the last one and ends at `rows`
        idx = torch.randint(0, max(V - 1, 1), (rows,), generator=g)
        idx[rows - max(1, min(rows // 4, 300)):] = V - 1
    elif pattern == "skip_min":
        skip = int(idx.min())
    elif pattern == "skip_max":
        skip = int(idx.max())
    elif pattern == "skip_only":
        idx[:] = V // 2
        skip = V // 2
    elif pattern == "skip_absent":
        absent = sorted(set(range(min(V, 64))) - set(idx.tolist()))
        skip = absent[0] if absent else V + 1
    elif pattern == "oob":                      # dropped: negative, >= V, beyond 32 bits, and valid rows moved by 2^19 (what a truncated key would alias)
        bad = torch.tensor([-1, V, -7, V + 3, (1 << 40) + 1, (1 << 19) + V // 2, -(1 << 33), (1 << 32)])
        at = torch.arange(rows) % 3 == 1 if rows > 1 else torch.ones(1, dtype=torch.bool)
        idx[at] = bad[torch.arange(int(at.sum())) % bad.numel()]
    elif pattern == "ends":
        idx = torch.where(torch.arange(rows) % 3 == 0, 0, V - 1)
    else:
        raise KeyError(pattern)
    return idx, skip


def table_fill(rows_index):
    """What a destination table holds before the call: non-zero-mean integers in [-100, 100] as a function of (row, col), any device."""
    r = rows_index.to(torch.int64)[:, None]
    c = torch.arange(D, device=rows_index.device)[None, :]
    return ((r * 7 + c * 3) % 201 - 100).to(F32)


def sc_build(c):
    key = ("sc",) + tuple(c)
    if key in _BUILT:
        return _BUILT[key]
    g = gen(*key)
    x = Inputs()
    x.idx, x.skip = sc_indices(c.rows, c.V, c.pattern, g)
    x.src = ints((c.rows, D), g, -64, 64).to(F32) if c.kind == "exact" else wide((c.rows, D), g)
    x.fill = 3.0 if c.V == SC_TOP else None      # the 1.6 GB table is a constant, not table_fill
    _BUILT[key] = x
    return x


def sc_contributing(idx, V, skip):
    return (idx >= 0) & (idx < V) & (idx != skip)


def sc_expected_rows(x, V, kind, fault=None, f=F64, order="asc", g=None):
    """-> (touched (k,) destination rows ascending, values (k, 768) fp32): what those rows hold afterwards; every other row keeps its fill.
    exact: fill + index_add_ in fp64 (f = fp32 / order: the CPU self-check evaluates it in fp32 in another order); order: fill + emulate_runs.
    Faults: "skipped_row_contributes", "run_absorbs_next" (the first row of the next destination is added to the run before it too)."""
    idx, src = x.idx, x.src
    ok = sc_contributing(idx, V, -1 if fault == "skipped_row_contributes" else x.skip)
    touched, inv = torch.unique(idx[ok], return_inverse=True)
    s = src[ok]
    if fault == "run_absorbs_next" and touched.numel() > 1:
        first_of_next = torch.tensor([int((inv == d).nonzero()[0]) for d in range(1, touched.numel())])
        s = torch.cat([s, s[first_of_next]], 0)
        inv = torch.cat([inv, torch.arange(touched.numel() - 1)], 0)
    fill = table_fill(touched) if x.fill is None else torch.full((touched.numel(), D), x.fill)
    if kind == "exact" and f == F64:
        acc = torch.zeros(touched.numel(), D, dtype=F64).index_add_(0, inv, s.to(F64))
        return touched, (fill.to(F64) + acc).to(F32)
    return touched, fill + emulate_runs(s, inv, touched.numel(), order, g)


def mod_build(rows, idx_mod, kind):
    key = ("mod", rows, idx_mod, kind)
    if key not in _BUILT:
        g = gen(*key)
        x = Inputs()
        x.idx, x.skip, x.fill = torch.arange(rows) % idx_mod, -1, None
        x.src = ints((rows, D), g, -64, 64).to(F32) if kind == "exact" else wide((rows, D), g)
        _BUILT[key] = x
    return _BUILT[key]


def mod_skip_build(rows, idx_mod, skip):
    """The position form's exact inputs with the rows of destination `skip` left out."""
    base = mod_build(rows, idx_mod, "exact")
    x = Inputs()
    x.idx, x.src, x.skip, x.fill = base.idx, base.src, skip, None
    return x


def table_expected(V, touched, values, guard=GUARD, fault=None):
    """The whole destination buffer on the CPU: (guard + V + guard, 768), table_fill in the table rows, SENTINEL in the guards."""
    buf = torch.full((guard + V + guard, D), SENTINEL, dtype=F32)
    buf[guard:guard + V] = table_fill(torch.arange(V))
    buf[guard + touched] = values
    if fault == "guard_overwritten":
        buf[guard + V, 0] = 0.0
    return buf


# ------------------------------------------------------------------------------------------------ gather_seq
GS_SHAPES = ((1, 1, 1, 1, 1), (6, 3, 5, 9, 11), (4, 4, 40, 197, 16), (2, 2, 1, 1, 8192))      # (Pt, Pv, Lt, Lv, S)
GS_PATTERNS = ("one_row", "identity", "some_unused")
GsCase = namedtuple("GsCase", "Pt Pv Lt Lv S pattern dt")       # dt: the 16-bit dtype of out_t / d_t, or F32 for none
GATHER_SEQ_CASES = tuple(GsCase(*s, p, dt) for s in GS_SHAPES for p in GS_PATTERNS for dt in DTS)


def gs_id(c):
    return "pt%d-pv%d-lt%d-lv%d-s%d-%s-%s" % (c.Pt, c.Pv, c.Lt, c.Lv, c.S, c.pattern, DT_NAME[c.dt])


def gs_indices(P, S, pattern, g):
    s = torch.arange(S)
    if pattern == "one_row":
        return torch.full((S,), P - 1)
    if pattern == "identity":
        return s % P
    used = torch.arange(0, P, 2)                # the odd pool rows stay unused
    return used[torch.randint(0, used.numel(), (S,), generator=g)]


def gs_build(c):
    """text / video pools with row-identifying fp32 values; ti / vi; the upstream gradients d32 (fp32) and d_t (c.dt, None for F32), once as
    integers in [-32, 32] ("exact") and once with a wide exponent spread ("order").  With d_t a pool row used by all S = 8192 sequences sums
    2 * 8192 terms: |x| <= 32 keeps that sum below 2^19, far inside the 2^24 bound that makes the order irrelevant."""
    key = ("gs",) + tuple(c[:6]) + (DT_NAME[c.dt],)
    if key in _BUILT:
        return _BUILT[key]
    g = gen(*key)
    x = Inputs()
    x.text = row_ident(c.Pt * c.Lt, D).to(F32).view(c.Pt, c.Lt, D)
    x.video = row_ident(c.Pv * c.Lv, D, row0=c.Pt * c.Lt).to(F32).view(c.Pv, c.Lv, D)
    x.ti, x.vi = gs_indices(c.Pt, c.S, c.pattern, g), gs_indices(c.Pv, c.S, c.pattern, g)
    n = c.S * (c.Lt + c.Lv)
    x.d32 = dict(exact=ints((n, D), g, -32, 32).to(F32), order=wide((n, D), g))
    x.d_t = dict(exact=None, order=None)
    if c.dt != F32:
        x.d_t = dict(exact=lossless(ints((n, D), g, -32, 32), c.dt), order=wide((n, D), g).to(c.dt))
    _BUILT[key] = x
    return x


def gs_forward_ref(x):
    return torch.cat([x.text[x.ti], x.video[x.vi]], 1).reshape(-1, D)


def gs_backward_ref(c, x):
    """fp64 autograd of the forward expression under the upstream gradient d32 + d_t (the exact inputs)."""
    t64, v64 = x.text.double().requires_grad_(True), x.video.double().requires_grad_(True)
    up = x.d32["exact"].double() + (0 if x.d_t["exact"] is None else x.d_t["exact"].double())
    (torch.cat([t64[x.ti], v64[x.vi]], 1).reshape(-1, D) * up).sum().backward()
    return t64.grad.to(F32), v64.grad.to(F32)


def gs_backward_emulated(c, x, kind="order", order="asc", swap=False, g=None):
    """Per pool row: from 0, ascending s over the sequences that used it, d32[s] then d_t[s] (swap: the other way round), fp32 adds; stored."""
    L = c.Lt + c.Lv
    d32 = x.d32[kind].view(c.S, L, D)
    d_t = None if x.d_t[kind] is None else x.d_t[kind].float().view(c.S, L, D)
    outs = []
    for idx, P, sl in ((x.ti, c.Pt, slice(0, c.Lt)), (x.vi, c.Pv, slice(c.Lt, L))):
        if d_t is None:
            terms, dest = d32[:, sl], idx
        else:
            pair = (d_t[:, sl], d32[:, sl]) if swap else (d32[:, sl], d_t[:, sl])
            terms = torch.stack(pair, 1).reshape((2 * c.S,) + tuple(d32[:, sl].shape[1:]))
            dest = idx.repeat_interleave(2)
        outs.append(emulate_runs(terms.contiguous(), dest, P, order, g))
    return outs


# ------------------------------------------------------------------------------------------------ patchify, cls_mean_bwd, gelu_bwd
PATCHIFY_SHAPES = ((1, 3, 16, 16), (1, 1, 16, 16), (2, 3, 16, 64), (2, 3, 64, 16), (3, 3, 32, 48))


def patchify_image(shape, dt):
    """Row-identifying pixels: the pixel's linear index (fp32 copy), or (index mod 129) - 64 where the output is 16-bit (exact there; 129 is
    coprime to every width and to 16, so neighbours in any direction differ)."""
    n = shape[0] * shape[1] * shape[2] * shape[3]
    v = torch.arange(n).view(shape)
    return (v if dt == F32 else v % 129 - 64).to(F32)


def patchify_ref(img):
    """(BT * N, C * 256): F.unfold's (BT, C*256, N) with the patch index moved in front."""
    BT, C = img.shape[:2]
    return F.unfold(img.double(), kernel_size=16, stride=16).transpose(1, 2).reshape(-1, C * 256)


CLS_MEAN_CASES = ((1, 1), (3, 4), (2, 128), (2, 3))       # (B, T); T = 3: 1 / T is not a power of two -> the fp32 restatement x * (1.0f / 3)


def cls_mean_ref(cls_rows, T):
    """dside[b*T + t] = cls_rows[b] / T.  T a power of two: exact in fp64; T = 3: the kernel's fp32 product x * (1.0f / T), restated."""
    inv = torch.ones((), dtype=F32) / T
    return (cls_rows.to(F32) * inv).repeat_interleave(T, 0)


# n: one chunk; one row; 8 elements more than one grid stride (4096 workgroups x 256 lanes x one 16-byte chunk: 4 fp32 or 8 16-bit elements)
GELU_GRID_CHUNKS = 4096 * 256
GELU_CASES = tuple((n, dt) for dt in DTS for n in (8, 3072, GELU_GRID_CHUNKS * (4 if dt == F32 else 8) + 8)) + ((GELU_GRID_CHUNKS * 4 + 8, BF16), (GELU_GRID_CHUNKS * 4 + 8, F16))
GELU_TOL = {F32: (1e-5, 1e-5), BF16: (1e-2, 1e-2), F16: (2e-3, 2e-3)}     # tests/test_hip_bwd_ops.py::test_transpose_gelu_misc
