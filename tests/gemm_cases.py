"""Exact-arithmetic cases for the GEMM family: alpro_gemm on its three kernels (128 x 128, persistent 256 x 256, 8-phase 256 x 256 with its
remainder launch and tail hand-over), alpro_gemm_batch, and the weight-gradient trio alpro_gemm_tn_acc / alpro_colsum_tn / alpro_colsum_acc.
Shared by tests/test_hip_gemm_exact.py (GPU) and tests/test_gemm_cases_cpu.py (CPU self-check); not collected itself, torch on the CPU only.

The idea: A and W are integers in [-3, 3] (exact in fp32, bf16 and fp16) and K <= 3072, so every product and every partial sum is an
integer below 2^24 and the fp32 accumulator is exact whatever the MFMA shape, the K-tile order, the split or the order of atomics.  The
epilogue stays on the same grid -- integer bias and residual, alpha a power of two, row scales from {0, 0.5, 1, 2}, integer saved factors,
dropout with p = 0.5 (keep scale 2) -- so an fp32 output must equal the fp64 reference bit for bit and a 16-bit output the reference rounded
ONCE to nearest-even.  A 16-bit output only shows a second rounding (or a wrong rounding mode) where the exact value is not representable:
[-3, 3] operands reach that range at no K of interest (bf16 needs |x| > 256, fp16 |x| > 2048), so the 16-bit-output cases carry an offset
INSIDE the product -- column 0 of W holds a signed multiple of 4 (256 .. 1020 for bf16, 2048 .. 4092 for fp16: exact in the dtype), which
row m multiplies by A[m, 0] in [-3, 3] -- and an integer bias on top where the epilogue has one.  tests/test_gemm_cases_cpu.py checks on
every run that each case does exercise what it claims.

The GELU family (GELU, GELU_SAVE_GRAD, GELU_BWD) is not exact: those cases keep exact pre-activations (alpha = 2^-j puts them inside
[-6, 6]) and are compared under the tolerances tests/test_hip_ops.py already uses; what each GELU form is held to over every 16-bit input,
the far tails and non-finite values is the subject of tests/gelu_cases.py.
"""
import math
import zlib
from collections import namedtuple

import torch

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
# include/alpro_hip.h (ALPRO_ACT_* / ALPRO_MAP_*); tests/test_hip_gemm_exact.py asserts they are alpro_amd.hip's
ACT_NONE, ACT_GELU, ACT_RELU, ACT_GELU_BWD, ACT_GELU_SAVE_GRAD, ACT_MUL_SAVED = 0, 1, 2, 3, 4, 5
MAP_IDENTITY, MAP_SKIP_CLS, MAP_FRAME_TOKENS, MAP_PATCH_EMBED = 0, 1, 2, 3
SENTINEL = -8192.0        # what output buffers hold before a launch: a power of two, exact in every dtype
GUARD_ROWS = 256          # rows behind every output view: a whole tile row of the largest kernel
DROP_P = 0.5
ROUTES = ("k128", "p256", "q8", "q8_rem", "q8_tail")   # 128 x 128; persistent 256; 8-phase; 8-phase + remainder launch; 8-phase + tail hand-over
ROUTE_OPTS = {"k128": (("gemm_tile", 128),), "p256": (("gemm_tile", 256), ("gemm_kind", 0)), "q8": (("gemm_tile", 256), ("gemm_kind", 1)),
              "q8_rem": (("gemm_tile", 256), ("gemm_kind", 1)), "q8_tail": (("gemm_tile", 256), ("gemm_kind", 1), ("gemm_grid", 8))}

# epilogue name -> what it switches on.  bias: integer bias; alpha: a power of two; scale: row scale (the case's group); res: fp32 residual;
# c2: "copy" = the pre-activation copy is written, "in" = a saved operand is read, "out" = gelu' is written; drop: dropout; map / bias2 / side
EPI = {
    "plain": {},
    "bias": dict(bias=True),
    "bias_alpha": dict(bias=True, alpha=0.5),
    "scale": dict(bias=True, scale=True),
    "res": dict(bias=True, res=True),
    "res_scale": dict(bias=True, scale=True, res=True),
    "relu": dict(bias=True, act=ACT_RELU),
    "relu_copy": dict(bias=True, act=ACT_RELU, c2="copy"),
    "mul_saved": dict(bias=True, act=ACT_MUL_SAVED, c2="in"),
    "gelu": dict(bias=True, act=ACT_GELU, inexact=True),
    "gelu_save": dict(bias=True, act=ACT_GELU_SAVE_GRAD, c2="out", inexact=True),
    "gelu_bwd": dict(bias=True, act=ACT_GELU_BWD, c2="in", inexact=True),
    "dropout": dict(bias=True, drop=True),
    "scale_drop": dict(bias=True, scale=True, drop=True),
    "skip_cls": dict(bias=True, res=True, map=MAP_SKIP_CLS),
    "skip_cls_bias2": dict(bias=True, res=True, scale=True, bias2=True, map=MAP_SKIP_CLS),
    "frame": dict(bias=True, res=True, map=MAP_FRAME_TOKENS),
    "patch": dict(res=True, map=MAP_PATCH_EMBED),
    "nan_row": dict(bias=True, nan_row=True),        # one NaN in the last valid row of A
}
# layout variants.  Every case already runs with its operands inside NaN-filled buffers (rows behind M and N) and its outputs inside
# sentinel-filled ones (GUARD_ROWS rows behind); these add to that:
#   wide_in   lda, ldw = K + 64 (NaN in the padding columns)            wide_out  ldc / ldr / ldc2 / ld_side = N + 8 / 16 / 24 / 32 (guard columns)
#   row1      A, W, C (and residual, C2) start at row 1 of their buffers   lda8      lda = K + 8: rows not 128-byte aligned (8-phase ineligible)
#   lda8_row1 lda8 with A starting at row 1: a base pointer off 128-byte alignment
LAYOUTS = ("tight", "wide_in", "wide_out", "row1", "lda8", "lda8_row1")

_CaseBase = namedtuple("Case", "route M N K dt out epi group layout map_dims variants tiled")


class Case(_CaseBase):
    """route: the kernel path the options force (ROUTES).  out: "same" (the operand dtype) or "f32".  group: row-scale group.  map_dims: (B, T, N)
    of a row-map case (M is then the map's row count).  variants: option settings, ((name, value), ...) each, that must all give the bits of the
    reference (the first one is the case's own route options).  tiled: the C2 buffer is in the 8-phase kernel's tile layout."""
    __slots__ = ()

    @property
    def id(self):
        s = "%s-%dx%dx%d-%s-%s-%s" % (self.route, self.M, self.N, self.K, DT_NAME[self.dt], "o32" if self.out == "f32" else "o16" if self.dt != F32 else "o32", self.epi)
        if self.group:
            s += "-g%d" % self.group
        if self.map_dims:
            s += "-b%dt%dn%d" % self.map_dims
        if self.tiled:
            s += "-tiled"
        if self.layout != "tight":
            s += "-" + self.layout
        if len(self.variants) > 1:
            s += "-v%d" % len(self.variants)
        if self.variants[0] != ROUTE_OPTS[self.route]:
            s += "-" + "_".join("%s%d" % (k.replace("gemm_", ""), v) for k, v in self.variants[0])
        return s

    @property
    def out_dtype(self):
        return F32 if self.out == "f32" else self.dt

    @property
    def exact(self):
        return not EPI[self.epi].get("inexact", False)

    @property
    def split_row(self):
        """First row of the second launch (remainder / tail hand-over), or None: the row from which the library sets m_off."""
        if self.route == "q8_rem":
            return self.M // 256 * 256
        if self.route == "q8_tail":
            return TAIL_FIRST_ROW
        return None


def case(route, M, N, K, dt, out="same", epi="plain", group=0, layout="tight", map_dims=None, variants=None, tiled=False, opts=None):
    base = tuple(opts) if opts is not None else ROUTE_OPTS[route]
    vs = (base,) + tuple(tuple(base) + tuple(v) for v in (variants or ()))
    if EPI[epi].get("map"):
        B, T, Np = map_dims
        M = {MAP_SKIP_CLS: B * Np * T, MAP_FRAME_TOKENS: B * T * (Np + 1), MAP_PATCH_EMBED: B * T * Np}[EPI[epi]["map"]]
    return Case(route, M, N, K, dt, "f32" if dt == F32 else out, epi, group, layout, map_dims, vs, tiled)


# ------------------------------------------------------------------------------------------------ the tables
K128_M, K128_N = (1, 127, 128, 129, 257), (2, 8, 100, 128, 132, 260)
P256_M, P256_N, P256_K = (1, 255, 256, 257, 384, 513), (8, 256, 264, 520), (128, 192, 768)
Q8_M, Q8_N, Q8_K = (256, 512, 512 + 16, 512 + 240, 512 + 8, 512 + 100), (256, 512), (256, 384, 768)
MAP_DIMS = ((2, 4, 9), (1, 1, 1))
TAIL_SHAPE = (10 * 256 + 64, 256, 2048)     # 11 tile rows on a grid of 8: R = 3, 5 * 3 <= 16 -> three row panels go to the 128 x 128 kernel
TAIL_FIRST_ROW = 8 * 256
HALF_SPLIT_SHAPE = (11 * 256 - 100, 256, 128)   # persistent kernel, grid 8: 3 tiles in the last round, 2 * 3 <= 8 -> half tiles, the last one partial
Q8_SAME_BITS = ((("gemm_sched", 0),), (("gemm_epi", 0),), (("gemm_grid", 8),), (("cu_budget", 64),))   # (cu_budget: the per-stream option)
TAIL_BOTH = ((("gemm_tail", 0),),)            # (the route options leave gemm_tail at its default, 1)
TUNES = ((("gemm_tune", 0),), (("gemm_tune", 2),))


def k_tiles_128(dt):
    """One K-tile of the 128 x 128 kernel (128 bytes of a row), two, three (an odd count) and 768."""
    k1 = 32 if dt == F32 else 64
    return (k1, 2 * k1, 3 * k1, 768)


def _outs(dt):
    return ("f32",) if dt == F32 else ("same", "f32")


def _epilogue_block(route, M, N, K, dt, groups_res, maps=True):
    """Every epilogue of the 128 x 128 and the persistent kernel at one shape, in both output dtypes."""
    cs = []
    for out in _outs(dt):
        cs += [case(route, M, N, K, dt, out, e) for e in ("plain", "bias_alpha", "relu_copy", "mul_saved", "gelu", "gelu_save", "gelu_bwd", "dropout")]
        cs += [case(route, M, N, K, dt, out, "res_scale", group=g) for g in groups_res]
        if maps:
            for dims in MAP_DIMS:
                cs += [case(route, 0, N, K, dt, out, e, map_dims=dims) for e in ("skip_cls", "frame", "patch")]
                cs.append(case(route, 0, N, K, dt, out, "skip_cls_bias2", group=5, map_dims=dims))
    return cs


def _build_gemm_cases():
    cs = []
    for dt in (F32, BF16, F16):
        k1 = k_tiles_128(dt)[1]
        # ---- 128 x 128: every M x N remainder pair at one K, every K at one ragged (M, N), every epilogue at a ragged shape (N % 8 == 0 for C2)
        cs += [case("k128", M, N, k1, dt, "same", "bias_alpha") for M in K128_M for N in K128_N]
        cs += [case("k128", 129, 100, K, dt, out, "plain") for K in k_tiles_128(dt) for out in _outs(dt)]
        cs += _epilogue_block("k128", 257, 136, k1, dt, (1, 7, 65))
        cs += [case("k128", 129, 8, k1, dt, "same", e) for e in ("relu_copy", "mul_saved", "gelu_save", "gelu_bwd")]
        # ---- persistent 256 x 256 (needs two K-tiles)
        cs += [case("p256", M, N, 128, dt, "same", "bias_alpha") for M in P256_M for N in P256_N]
        cs += [case("p256", 257, 264, K, dt, out, "plain") for K in P256_K for out in _outs(dt)]
        cs += _epilogue_block("p256", 513, 264, 128, dt, (1, 7, 65))
        Mh, Nh, Kh = HALF_SPLIT_SHAPE
        cs += [case("p256", Mh, Nh, Kh, dt, "same", "bias", variants=TAIL_BOTH, opts=ROUTE_OPTS["p256"] + (("gemm_grid", 8),)),
               case("p256", Mh, Nh, Kh, dt, "f32", "res_scale", group=1569, variants=TAIL_BOTH, opts=ROUTE_OPTS["p256"] + (("gemm_grid", 8),)),
               case("p256", Mh, Nh, Kh, dt, "same", "gelu_save", variants=TAIL_BOTH, opts=ROUTE_OPTS["p256"] + (("gemm_grid", 8),))]
        # ---- layout variants and non-finite propagation: one plain and one residual case per kernel
        for route, (M, N, K) in (("k128", (129, 100, k1)), ("p256", (257, 264, 128))):
            for lay in ("wide_in", "wide_out", "row1"):
                cs += [case(route, M, N, K, dt, "same", "plain", layout=lay), case(route, M, N, K, dt, "f32", "res_scale", group=7, layout=lay)]
            cs.append(case(route, M, N, K, dt, "same", "relu_copy", layout="wide_out"))
            cs.append(case(route, M, N, K, dt, "same", "nan_row"))
    cs += [case("p256", 257, 264, K, BF16, "same", "plain", variants=TUNES) for K in P256_K]
    for dt in (BF16, F16):
        def route_of(M):
            return "q8" if M % 16 == 0 else "q8_rem"
        # ---- 8-phase: every M x N at one K, every K at an in-launch and a second-launch remainder
        cs += [case(route_of(M), M, N, 256, dt, "same", "plain", variants=Q8_SAME_BITS) for M in Q8_M for N in Q8_N]
        cs += [case(route_of(M), M, N, K, dt, "same", "bias", variants=Q8_SAME_BITS) for (M, N) in ((528, 256), (612, 512)) for K in Q8_K]
        for M in (512 + 16, 512 + 100):
            r = route_of(M)
            cs += [case(r, M, 256, 256, dt, "same", e, variants=Q8_SAME_BITS) for e in ("bias", "relu", "relu_copy", "mul_saved", "gelu", "gelu_save", "dropout")]
            cs += [case(r, M, 256, 256, dt, "same", "scale", group=g, variants=Q8_SAME_BITS) for g in (8, 9, 16, 197)]
            cs += [case(r, M, 256, 256, dt, "f32", "res_scale", group=g, variants=Q8_SAME_BITS) for g in (16, 17, 197)]
            cs += [case(r, M, 256, 256, dt, "same", "scale_drop", group=g, variants=Q8_SAME_BITS) for g in (9, 197)]
            # groups the 8-phase epilogues do not take: the launcher must fall through to the persistent kernel with the same bits
            cs += [case("p256", M, 256, 256, dt, "same", "scale", group=7, opts=ROUTE_OPTS["q8"]), case("p256", M, 256, 256, dt, "f32", "res_scale", group=15, opts=ROUTE_OPTS["q8"])]
        cs += [case("q8", 528, 256, 256, dt, "same", e, tiled=True) for e in ("mul_saved", "gelu_save")]
        # ---- tail hand-over (gemm_tail 0 and 1): 16-bit output, row scale, fp32 residual + row scale with a group cut by the hand-over row, dropout
        Mt, Nt, Kt = TAIL_SHAPE
        cs += [case("q8_tail", Mt, Nt, Kt, dt, "same", "bias", variants=TAIL_BOTH), case("q8_tail", Mt, Nt, Kt, dt, "same", "scale", group=197, variants=TAIL_BOTH),
               case("q8_tail", Mt, Nt, Kt, dt, "f32", "res_scale", group=1569, variants=TAIL_BOTH), case("q8_tail", Mt, Nt, Kt, dt, "f32", "res_scale", group=17, variants=TAIL_BOTH),
               case("q8_tail", Mt, Nt, Kt, dt, "same", "scale_drop", group=1569, variants=TAIL_BOTH)]
        # ---- ineligible on purpose: unaligned operand rows, a base pointer off 128 bytes, K = 192, N = 264 -> the persistent kernel
        cs += [case("p256", 528, 256, 256, dt, "same", "bias", layout="lda8", opts=ROUTE_OPTS["q8"]), case("p256", 528, 256, 256, dt, "same", "bias", layout="lda8_row1", opts=ROUTE_OPTS["q8"]),
               case("p256", 528, 256, 192, dt, "same", "bias", opts=ROUTE_OPTS["q8"]), case("p256", 528, 264, 256, dt, "same", "bias", opts=ROUTE_OPTS["q8"])]
        for lay in ("wide_in", "wide_out", "row1"):
            cs += [case("q8", 528, 256, 256, dt, "same", "plain", layout=lay), case("q8", 528, 256, 256, dt, "f32", "res_scale", group=17, layout=lay),
                   case("q8_rem", 612, 256, 256, dt, "f32", "res_scale", group=17, layout=lay)]
        cs += [case("q8", 528, 256, 256, dt, "same", "gelu_save", layout="wide_out"), case("q8", 528, 256, 256, dt, "same", "nan_row"), case("q8_rem", 612, 256, 256, dt, "same", "nan_row")]
    by_id = {c.id: c for c in cs}      # (a cell that two of the lists above name is one case)
    assert all(by_id[c.id] == c for c in cs)
    return tuple(by_id.values())


GEMM_CASES = _build_gemm_cases()

# alpro_gemm_batch: one launch of five jobs of unequal shape (the grid is sized by the largest, the others return early): (M, N, K, epilogue, out)
BATCH_JOBS = ((1, 8, 64, "bias", "same"), (130, 200, 128, "bias_alpha", "f32"), (128, 128, 768, "res", "f32"), (257, 132, 64, "plain", "same"), (768, 768, 768, "bias_alpha", "same"))

# weight-gradient GEMM: stages are 32 tokens, tiles 256 wide.  (33, 100, 20) adds what the issue's N and K (all multiples of 8) leave out: columns
# between N / K and the next multiple of 8, which the kernel reads as part of a whole 16-byte chunk
TN_M, TN_N, TN_K = (1, 31, 32, 33, 130, 1000), (8, 256, 264, 520), (8, 256, 264)
TN_SHAPES = tuple((M, N, K) for M in TN_M for N in TN_N for K in TN_K) + ((33, 100, 20),)
TN_SPLITS = (0, 1, 2, 3, 7, 64)     # 64 exceeds the stage count at M = 130


# ------------------------------------------------------------------------------------------------ builders
def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(shape, g, lo=-3, hi=3):
    """Uniform integers in [lo, hi] as fp64."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(F64)


def lossless(x, dt):
    y = x.to(dt)
    assert torch.equal(y.to(F64), x.to(F64)), "operand is not exact in %s" % dt
    return y


def offset_column(N, dt, g):
    """The rounding exercise of the 16-bit-output cases: signed multiples of 4 that the dtype holds exactly and that lift |out| into the range
    where integers are no longer representable (bf16: 8 significant bits, fp16: 11)."""
    lo, hi = (64, 255) if dt == BF16 else (512, 1023)
    mag = 4.0 * torch.randint(lo, hi + 1, (N,), generator=g).to(F64)
    return mag * (2.0 * torch.randint(0, 2, (N,), generator=g).to(F64) - 1.0)


def row_scales(n_groups, g, nonzero_at=None):
    """From {0, 0.5, 1, 2}: neighbours differ (a scale taken from the next group shows), at least one 0 and one value that is not 1; the group
    `nonzero_at` (the one a split launch starts in) keeps its rows visible."""
    vals = (0.0, 0.5, 1.0, 2.0)
    rs = []
    for i in range(n_groups):
        ok = [v for v in vals if (not rs or v != rs[-1]) and not (i == nonzero_at and v == 0.0) and not (n_groups == 1 and v == 1.0)]
        rs.append(ok[int(torch.randint(0, len(ok), (1,), generator=g))])
    if n_groups >= 2 and 0.0 not in rs:      # (no zero anywhere: planting one keeps every neighbour pair different)
        free = [i for i in range(n_groups) if i != nonzero_at]
        rs[free[int(torch.randint(0, len(free), (1,), generator=g))]] = 0.0
    return torch.tensor(rs, dtype=F32)


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def keep_mask(seed, rows, N):
    """(rows, N) {0, 1} fp64: the dropout hash of element m * N + n (common.hpp drop_keep, restated in tests/test_hip_bwd_ops.py)."""
    from tests.test_hip_bwd_ops import _keep_mask
    return _keep_mask(seed, rows * N, DROP_P).view(rows, N).to(F64)


def map_rows(mode, dims, M):
    """-> (out_rows, orow (M,), rrow (M,), is_side (M,)): include/alpro_hip.h's row maps; side rows carry the side-buffer row in orow."""
    m = torch.arange(M)
    if mode == MAP_IDENTITY:
        return M, m, m, torch.zeros(M, dtype=torch.bool)
    B, T, Np = dims
    S = 1 + Np * T
    if mode == MAP_SKIP_CLS:
        o = m + m // (Np * T) + 1
        return B * S, o, o, torch.zeros(M, dtype=torch.bool)
    if mode == MAP_FRAME_TOKENS:
        bt, j = m // (Np + 1), m % (Np + 1)
        b, t = bt // T, bt % T
        o = b * S + 1 + (j - 1) * T + t
        side = j == 0
        return B * S, torch.where(side, bt, o), o, side
    bt, n = m // Np, m % Np
    b, t = bt // T, bt % T
    return B * S, b * S + 1 + n * T + t, n * T + t, torch.zeros(M, dtype=torch.bool)


class Inputs:
    pass


_BUILT = {}


def build(c):
    """The operands of a case (CPU tensors in the dtypes the library takes) -- built once per case and shared, never modified."""
    if c.id in _BUILT:
        return _BUILT[c.id]
    for attempt in range(256):
        x = _draw(c, attempt)
        if not (c.exact and c.out_dtype != F32):
            break
        # a 16-bit-output case must exercise the rounding (tests/test_gemm_cases_cpu.py): the few-element shapes (1 x 2, 1 x 8) only do
        # under some draws, so the draw is repeated -- judged by the reference alone -- until it does
        r = x.ref["out"][(x.ref["out"] != SENTINEL).any(1) & ~x.ref["out"].isnan().any(1)]
        if float((~representable(r, c.out_dtype)).double().mean()) >= 0.05 and bool(exact_ties(r, c.out_dtype).any()):
            break
    _BUILT[c.id] = x
    return x


def _draw(c, attempt):
    e = EPI[c.epi]
    g = gen("gemm", c.route, c.M, c.N, c.K, DT_NAME[c.dt], c.out, c.epi, c.group, c.map_dims, attempt)
    x = Inputs()
    x.case, x.epi = c, e
    a, w = ints((c.M, c.K), g), ints((c.N, c.K), g)
    if c.exact and c.out_dtype != F32:
        w[:, 0] = offset_column(c.N, c.dt, g)
    if e.get("nan_row"):
        a[c.M - 1, (7 * c.M) % c.K] = float("nan")
    x.a, x.w = (a.to(c.dt) if e.get("nan_row") else lossless(a, c.dt)), lossless(w, c.dt)
    x.alpha = e.get("alpha", 1.0)
    x.bias = None
    if e.get("inexact"):      # exact pre-activations inside [-6, 6]: the accumulator's deviation is 4 sqrt(K)
        x.alpha = 2.0 ** -round(math.log2(4.0 * math.sqrt(c.K)))
        x.bias = ints((c.N,), g, -1, 1).to(F32)
    elif e.get("bias"):
        x.bias = ints((c.N,), g, -5, 5).to(F32)
    x.act = e.get("act", ACT_NONE)
    x.map_mode = e.get("map", MAP_IDENTITY)
    x.out_rows, x.orow, x.rrow, x.is_side = map_rows(x.map_mode, c.map_dims, c.M)
    _, T, Np = c.map_dims or (0, 0, 0)
    x.map_p0, x.map_p1 = (0, 0) if x.map_mode == MAP_IDENTITY else (Np * T, 0) if x.map_mode == MAP_SKIP_CLS else (T, Np)
    x.row_scale = row_scales((c.M + c.group - 1) // c.group, g, None if c.split_row is None else c.split_row // c.group) if e.get("scale") else None
    x.residual = None
    if e.get("res"):
        rr = c.map_dims[2] * c.map_dims[1] if x.map_mode == MAP_PATCH_EMBED else x.out_rows
        x.residual = ints((rr, c.N), g, -50, 50).to(F32)
    x.side_rows = c.map_dims[0] * c.map_dims[1] if x.map_mode == MAP_FRAME_TOKENS else 0
    x.bias2 = ints((c.N,), g, -5, 5).to(F32) if e.get("bias2") else None
    x.saved = None
    if e.get("c2") == "in":      # MUL_SAVED: integer factors; GELU_BWD: saved pre-activations on a 2^-5 grid inside [-4, 4]
        x.saved = lossless(ints((c.M, c.N), g) if x.act == ACT_MUL_SAVED else ints((c.M, c.N), g, -128, 128) / 32.0, c.dt)
    x.drop_seed = 1 + zlib.crc32(c.id.encode()) % 100000 if e.get("drop") else 0
    x.ref = reference(x)
    return x


def reference(x, fault=None, f=F64, perm=None):
    """fp64 of  C[map(m)] = residual + row_scale * act(alpha * A W^T + bias) [+ bias2]  -> dict(out=(out_rows, N) with SENTINEL in the rows the
    map does not reach, c2=(M, N) or None, side=(side_rows, N) or None, pre=the pre-activations, products=sum_k |a w|).
    fault: one deliberate corruption -- "scale_row_off_by_one" (row scale of row m + 1), "bias_after_rounding" (the bias added to the value
    already rounded to the output dtype), "dropout_without_m_off" (the second launch of a split hashes rows relative to its own first row).
    f, perm: evaluate in another float type with the K columns taken in another order (the CPU self-check: fp32 in any order equals fp64)."""
    c, e = x.case, x.epi
    a, w = x.a.to(f), x.w.to(f)
    if perm is not None:
        a, w = a[:, perm].contiguous(), w[:, perm].contiguous()
    acc = a @ w.T
    bias = x.bias.to(f) if x.bias is not None else torch.zeros(c.N, dtype=f)
    late_bias = fault == "bias_after_rounding"
    pre = x.alpha * acc + (0.0 if late_bias else bias)
    c2 = None
    if e.get("c2") == "copy":
        c2 = pre.clone()
    if x.act == ACT_RELU:
        v = pre.clamp(min=0.0)
    elif x.act == ACT_MUL_SAVED:
        v = pre * x.saved.to(f)
    elif x.act == ACT_GELU:
        v = gelu64(pre)
    elif x.act == ACT_GELU_SAVE_GRAD:
        v, c2 = gelu64(pre), gelu_grad64(pre)
    elif x.act == ACT_GELU_BWD:
        v = pre * gelu_grad64(x.saved.to(f))
    else:
        v = pre
    m = torch.arange(c.M)
    if x.row_scale is not None:
        mm = (m + 1).clamp(max=c.M - 1) if fault == "scale_row_off_by_one" else m
        v = v * x.row_scale.to(f)[mm // c.group][:, None]
    if x.drop_seed:
        keep = keep_mask(x.drop_seed, c.M, c.N).to(f)
        if fault == "dropout_without_m_off" and c.split_row is not None:
            keep = torch.cat([keep[:c.split_row], keep[:c.M - c.split_row]], 0)
        v = v * keep / (1.0 - DROP_P)
    if x.bias2 is not None:
        v = v + x.bias2.to(f)
    if late_bias:
        v = v.to(c.out_dtype).to(f) + bias
    main = ~x.is_side
    if x.residual is not None:
        v = torch.where(main[:, None], v + x.residual.to(f)[x.rrow.clamp(min=0)], v)
    out = torch.full((x.out_rows, c.N), SENTINEL, dtype=f)
    out[x.orow[main]] = v[main]
    side = None
    if x.side_rows:
        side = torch.full((x.side_rows, c.N), SENTINEL, dtype=f)
        side[x.orow[x.is_side]] = v[x.is_side]
    return dict(out=out, c2=c2, side=side, pre=pre, products=a.abs() @ w.abs().T)


def matches(got, ref64, dt):
    """THE comparison of the exact cases: the kernel's output (any device) against the fp64 reference rounded once to the output dtype
    (nearest-even, torch's conversion), every element, zero tolerance."""
    return torch.equal(got.detach().cpu(), ref64.to(dt))


def poisoned(t, rows, cols, row0, fill=float("nan"), device=None):
    """-> a view holding t's values inside a larger buffer of (row0 + t.shape[0] + rows, t.shape[1] + cols) elements whose other elements
    are `fill`: NaN for operands and fp32 side inputs, SENTINEL for outputs.  The buffer (view._base) goes to `device` whole."""
    R, C = t.shape
    buf = torch.full((row0 + R + rows, C + cols), fill, dtype=t.dtype)
    buf[row0:row0 + R, :C] = t
    if device is not None:
        buf = buf.to(device)
    return buf[row0:row0 + R, :C]


def poisoned_vec(t, extra, fill=float("nan"), device=None):
    """A 1-D operand (bias, row scales) in front of `extra` poisoned elements."""
    buf = torch.full((t.numel() + extra,), fill, dtype=t.dtype)
    buf[:t.numel()] = t
    if device is not None:
        buf = buf.to(device)
    return buf[:t.numel()]


def representable(ref64, dt):
    return ref64.to(dt).to(F64) == ref64


def exact_ties(ref64, dt):
    """Elements exactly half way between two neighbours of dt: the candidates below and above (nextafter in dt, via the bit pattern) are
    equally far."""
    r = ref64.to(dt)
    bits = r.view(torch.int16).to(torch.int32)
    up = ((bits + 1).to(torch.int16)).view(dt).to(F64)
    dn = ((bits - 1).to(torch.int16)).view(dt).to(F64)
    rr = r.to(F64)
    other = torch.where(ref64.abs() > rr.abs(), up, dn)     # the neighbour on the far side of the exact value (sign-magnitude patterns: +1 = away from zero)
    return (ref64 != rr) & ((ref64 - rr).abs() == (ref64 - other).abs())


# ------------------------------------------------------------------------------------------------ weight-gradient GEMM
def tn_inputs(M, N, K, dt):
    """a (M, N), b (M, K) integers in [-3, 3] in dt; c0 (N, K) and the colsum seed integers (fp32) -> and the fp64 references."""
    g = gen("tn", M, N, K, DT_NAME[dt])
    a, b = ints((M, N), g), ints((M, K), g)
    c0, cs0 = ints((N, K), g, -100, 100), ints((N,), g, -100, 100)
    return dict(a=lossless(a, dt), b=lossless(b, dt), c0=c0.to(F32), cs0=cs0.to(F32), ref_c=c0 + a.T @ b, ref_cs=cs0 + a.sum(0), products=a.abs().T @ b.abs())
