"""CPU self-check of tests/movement_cases.py: the cases test what they claim, so that none can pass vacuously on the GPU
(tests/test_hip_movement_exact.py) -- the exact cases are exact in fp32 in any summation order, the 16-bit ones survive the cast, the
order-sensitive inputs do tell summation orders apart, the row maps of the reference are the model's rearranges, and the comparison used on
the GPU rejects seven planted faults."""
import pytest
import torch

from tests import movement_cases as mc
from tests.gemm_cases import BF16, F16, F32, F64, MAP_FRAME_TOKENS, MAP_IDENTITY, MAP_PATCH_EMBED, MAP_SKIP_CLS, gen, ints

D, G = mc.D, mc.GUARD
GC_INPUTS = [c for c in mc.GATHER_CAST_CASES if c.dt == F32]      # (the three output dtypes of a case share their inputs)
SC_EXACT = [c for c in mc.ORDERED_SCATTER_CASES if c.kind == "exact"]
SC_OTHER = [c for _, cases in mc.OTHER_ROUTE_CASES.values() for c in cases]      # (torch's index_put_ and the atomic kernel: exact inputs too)
SC_ORDER = [c for c in mc.ORDERED_SCATTER_CASES if c.kind == "order"]
GS_INPUTS = [c for c in mc.GATHER_SEQ_CASES]


def lossless_in_16_bit(t):
    return all(torch.equal(t.to(dt).to(F64), t.to(F64)) for dt in (BF16, F16))


def tells_apart(a, b, counts):
    """Of the rows that received at least 3 terms: the share in which the two summation orders differ in at least one bit -> (share, rows)."""
    rows = (counts >= 3).nonzero().view(-1)
    if rows.numel() == 0:
        return 1.0, 0
    differ = (a[rows] != b[rows]).reshape(rows.numel(), -1).any(1)
    return float(differ.double().mean()), rows.numel()


# ------------------------------------------------------------------------------------------------ the case lists hold what the issue names
def test_case_lists_cover_the_named_shapes_and_routes():
    assert {(c.R, c.C) for c in mc.TRANSPOSE_CASES} == {(R, C) for R in (1, 63, 64, 65, 129) for C in (1, 63, 64, 65, 200)}
    assert any(c.R == 1 and c.pad_to == 256 for c in mc.TRANSPOSE_CASES)           # three all-zero tiles
    assert {(c.din, c.dout) for c in mc.TRANSPOSE_CASES} == {(F32, F32), (F32, BF16), (F32, F16), (BF16, BF16), (F16, F16)}
    mixed = [j[:2] for j in mc.TB_TABLES["mixed"]]
    assert set(mixed) == {(1, 1), (64, 64), (65, 63), (768, 3072), (3072, 768), (200, 300)}
    one_tile = [R <= 64 and C <= 64 for R, C in mixed]
    assert one_tile[0] and one_tile[-1] and any(one_tile[i] and not one_tile[i - 1] and not one_tile[i + 1] and min(mixed[i - 1] + mixed[i + 1]) >= 768 for i in range(1, len(mixed) - 1))
    assert len(mc.TB_TABLES["many"]) == 130 and len(mc.TB_TABLES["one"]) == 1
    assert any(e == 0 for _, _, e in mc.TB_MIXED) and any(e > 0 for _, _, e in mc.TB_MIXED)
    for mode in (MAP_SKIP_CLS, MAP_FRAME_TOKENS, MAP_PATCH_EMBED):
        assert {c.dims for c in mc.GATHER_CAST_CASES if c.mode == mode} == set(mc.GC_DIMS)
    assert {c.rows for c in mc.GATHER_CAST_CASES if c.mode == MAP_IDENTITY} == {1, 2, 7, 8191}
    for mode in (MAP_IDENTITY, MAP_SKIP_CLS, MAP_FRAME_TOKENS, MAP_PATCH_EMBED):
        for dt in mc.DTS:
            mine = [c for c in mc.GATHER_CAST_CASES if c.mode == mode and c.dt == dt]
            for shape in {(c.dims, c.rows) for c in mine}:
                here = [c for c in mine if (c.dims, c.rows) == shape]
                assert {(c.colsum, c.det) for c in here} == {(s, d) for s in mc.GC_COLSUMS for d in (True, False)}, (mode, shape)
                assert {c.drop for c in here} == {False, True} and 0 in {c.group for c in here}
                if shape[0] is not None:
                    B, T, N = shape[0]
                    assert {1, T, N + 1, 1 + N * T} <= {c.group for c in here}
                    assert any(c.group and (c.rows // B) % c.group and c.group not in (1, T, N + 1, 1 + N * T) for c in here)
    assert len({mc.gc_id(c) for c in mc.GATHER_CAST_CASES}) == len(mc.GATHER_CAST_CASES)
    assert {c.rows for c in SC_EXACT} == {1, 2, 5, 4096, 8191, 8192} and {c.V for c in SC_EXACT} == {1, 7, 30522, (1 << 19) - 1}
    assert {c.pattern for c in SC_EXACT} == set(mc.SC_PATTERNS) | {"ends"}
    assert all(c.rows <= 8192 and c.V < (1 << 19) for c in mc.ORDERED_SCATTER_CASES)


# ------------------------------------------------------------------------------------------------ exact in fp32 in any order; lossless in 16 bits
def test_transpose_inputs_are_exact():
    for c in mc.TRANSPOSE_CASES:
        t = mc.transpose_inputs(c)
        x = t["x"]
        assert torch.equal(x.to(c.din).to(c.dout).to(F64), x), mc.tr_id(c)
        assert float(t["colsum0"].abs().min()) >= 1 and float(t["colsum0"].abs().max() + x.abs().sum(0).max()) < mc.LIMIT
        perm = torch.randperm(c.R, generator=gen("perm", mc.tr_id(c)))
        cs32 = t["colsum0"] + mc.seq_sum(x.to(F32)[perm])
        assert cs32.dtype == F32 and torch.equal(cs32.to(F64), t["colsum"])
        if (c.din, c.dout) == (F32, F32) and c.R > 1 and c.C > 1:
            assert x.unique().numel() == x.numel()           # every element names its place
    for name, jobs in mc.TB_TABLES.items():
        for j, (R, C, extra) in enumerate(jobs):
            assert extra % 64 == 0
            assert lossless_in_16_bit(mc.matrix(R, C, F32, BF16, name, j))
            x = mc.matrix(R, C, F32, F32, name, j)
            assert torch.equal(x.to(F32).to(F64), x) and (x.unique().numel() == x.numel())


@pytest.mark.parametrize("c", GC_INPUTS, ids=[mc.gc_id(c) for c in GC_INPUTS])
def test_gather_cast_case_is_exact_in_fp32_in_any_summation_order(c):
    x = mc.gc_build(c)
    ref = x.ref
    assert ref["total"] / ref["unit"] < mc.LIMIT and c.rows <= 8192
    assert lossless_in_16_bit(ref["out"])
    r32 = mc.gc_reference(c, x, f=F32, perm=torch.randperm(c.rows, generator=gen("perm", mc.gc_id(c))))
    for k in ("out", "colsum", "pre"):
        assert r32[k].dtype == F32 and torch.equal(r32[k].to(F64), ref[k]), k
    if c.drop:      # the mask does drop and does keep
        kept = float(mc.keep_rows(x.drop_seed, c.rows).mean())
        assert 0.4 < kept < 0.6
    if c.group and c.rows > c.group:
        assert x.row_scale.unique().numel() > 1 and bool((x.row_scale[1:] != x.row_scale[:-1]).all())


@pytest.mark.parametrize("c", SC_EXACT + SC_OTHER, ids=[mc.sc_id(c) for c in SC_EXACT] + ["other-" + mc.sc_id(c) for c in SC_OTHER])
def test_scatter_case_is_exact_in_fp32_in_any_summation_order(c):
    x = mc.sc_build(c)
    touched, ref = mc.sc_expected_rows(x, c.V, "exact")
    ok = mc.sc_contributing(x.idx, c.V, x.skip)
    terms = int(torch.bincount(torch.unique(x.idx[ok], return_inverse=True)[1]).max()) if bool(ok.any()) else 0      # of the fullest destination row
    assert terms <= 8192 and c.kind == "exact" and float(x.src.abs().max()) * terms + 100 < mc.LIMIT
    t32, r32 = mc.sc_expected_rows(x, c.V, "exact", f=F32, order="random", g=gen("order", mc.sc_id(c)))
    assert torch.equal(t32, touched) and torch.equal(r32, ref)
    assert touched.numel() == x.idx[ok].unique().numel()
    # the pattern is what its name says
    if c.pattern == "oob":
        low, high = bool((x.idx < 0).any()), bool((x.idx >= c.V).any())
        assert (low and high if c.rows >= 5 else low or high) and int(ok.sum()) < c.rows
    else:
        assert bool(((x.idx >= 0) & (x.idx < c.V)).all())
    if c.pattern in ("skip_min", "skip_max", "skip_only") or (c.pattern == "mix" and c.rows >= 40):
        assert bool((x.idx == x.skip).any())
        assert x.skip == {"skip_min": int(x.idx.min()), "skip_max": int(x.idx.max())}.get(c.pattern, x.skip)
    if c.pattern == "skip_only":
        assert touched.numel() == 0
    if c.pattern == "skip_absent":
        assert x.skip >= 0 and not bool((x.idx == x.skip).any())
    if c.pattern == "top_last":
        assert int(x.idx[-1]) == c.V - 1 == int(x.idx.max())
    if c.pattern == "perm":
        assert touched.numel() == c.rows
    if c.pattern == "ends":
        assert touched.tolist() == [0, c.V - 1]


@pytest.mark.parametrize("c", SC_ORDER, ids=[mc.sc_id(c) for c in SC_ORDER])
def test_ordered_scatter_inputs_tell_summation_orders_apart(c):
    x = mc.sc_build(c)
    touched, asc = mc.sc_expected_rows(x, c.V, "order")
    ok = mc.sc_contributing(x.idx, c.V, x.skip)
    counts = torch.bincount(torch.unique(x.idx[ok], return_inverse=True)[1], minlength=touched.numel())
    for other in ("desc", "random"):
        _, o = mc.sc_expected_rows(x, c.V, "order", order=other, g=gen("order", mc.sc_id(c)))
        share, n = tells_apart(asc, o, counts)
        assert n > 0 and share >= 0.5, (other, share, n)


@pytest.mark.parametrize("rows,idx_mod", mc.MOD_CASES)
def test_position_scatter_inputs(rows, idx_mod):
    x = mc.mod_build(rows, idx_mod, "exact")
    touched, ref = mc.sc_expected_rows(x, idx_mod, "exact")
    _, r32 = mc.sc_expected_rows(x, idx_mod, "exact", f=F32, order="random", g=gen("order", rows, idx_mod))
    assert torch.equal(r32, ref) and touched.tolist() == list(range(min(rows, idx_mod))) and idx_mod <= mc.MOD_TABLE_ROWS
    counts = torch.bincount(x.idx, minlength=idx_mod)[touched]
    if int(counts.max()) >= 3:
        y = mc.mod_build(rows, idx_mod, "order")
        _, asc = mc.sc_expected_rows(y, idx_mod, "order")
        for other in ("desc", "random"):
            share, n = tells_apart(asc, mc.sc_expected_rows(y, idx_mod, "order", order=other, g=gen("order", rows, idx_mod))[1], counts)
            assert n > 0 and share >= 0.5
    assert {(5120, 40), (130, 33)} <= {m for m in mc.MOD_CASES if (m[0] + m[1] - 1) // m[1] >= 3}


@pytest.mark.parametrize("rows,idx_mod,skip", mc.MOD_SKIP_CASES)
def test_position_scatter_with_skip_inputs(rows, idx_mod, skip):
    """idx None with skip_idx >= 0: exact in fp32 in any order, the skipped destination is (in all cases but one) one that rows do reach, and skipping it changes the result."""
    x = mc.mod_skip_build(rows, idx_mod, skip)
    touched, ref = mc.sc_expected_rows(x, idx_mod, "exact")
    _, r32 = mc.sc_expected_rows(x, idx_mod, "exact", f=F32, order="random", g=gen("order", rows, idx_mod, skip))
    terms = (rows + idx_mod - 1) // idx_mod
    assert torch.equal(r32, ref) and terms <= 8192 and 64 * terms + 100 < mc.LIMIT
    reached = skip < min(rows, idx_mod)          # (5, 7, 6) skips a destination that no row reaches: nothing may change
    assert 0 <= skip < idx_mod <= mc.MOD_TABLE_ROWS and skip not in touched.tolist() and touched.numel() == min(rows, idx_mod) - reached
    t4, v4 = mc.sc_expected_rows(x, idx_mod, "exact", fault="skipped_row_contributes")
    assert mc.same(mc.table_expected(mc.MOD_TABLE_ROWS, t4, v4), mc.table_expected(mc.MOD_TABLE_ROWS, touched, ref)) != reached
    assert sum(k < min(r, m) for r, m, k in mc.MOD_SKIP_CASES) >= 3
    assert set(mc.OTHER_ROUTES) == set(mc.OTHER_ROUTE_CASES) | set(mc.MOD_SKIP_ROUTES) and set(mc.MOD_SKIP_ROUTES.values()) == {True, False}


@pytest.mark.parametrize("c", GS_INPUTS, ids=[mc.gs_id(c) for c in GS_INPUTS])
def test_gather_seq_inputs(c):
    x = mc.gs_build(c)
    assert c.S <= 8192 and bool((x.ti < c.Pt).all()) and bool((x.vi < c.Pv).all())
    pools = torch.cat([x.text.view(-1, D), x.video.view(-1, D)])
    assert pools.unique().numel() == pools.numel()
    # exact: fp32 in a random order equals the fp64 autograd reference; at most 2 * 8192 terms of at most 32 each
    terms = c.S * (1 if c.dt == F32 else 2)
    assert terms * 32 < mc.LIMIT
    ref = mc.gs_backward_ref(c, x)
    for r, e in zip(ref, mc.gs_backward_emulated(c, x, kind="exact", order="random", g=gen("order", mc.gs_id(c)))):
        assert torch.equal(r, e)
    if c.dt != F32:
        assert torch.equal(x.d_t["exact"].to(F64).to(c.dt), x.d_t["exact"])
    # order: ascending differs from descending, from a random order and from d_t before d32
    asc = mc.gs_backward_emulated(c, x)
    others = {o: mc.gs_backward_emulated(c, x, order=o, g=gen("order", mc.gs_id(c))) for o in ("desc", "random")}
    swapped = mc.gs_backward_emulated(c, x, swap=True) if c.dt != F32 else None
    per_s = 1 if c.dt == F32 else 2
    seen = 0
    for k, (idx, P) in enumerate(((x.ti, c.Pt), (x.vi, c.Pv))):
        counts = torch.bincount(idx, minlength=P) * per_s
        for other in ("desc", "random"):
            share, n = tells_apart(asc[k], others[other][k], counts)
            assert share >= 0.5, (other, share, n)
            seen += n
        if c.dt != F32:
            share, n = tells_apart(asc[k], swapped[k], counts)      # (a + b = b + a: it takes two sequences)
            assert (n > 0 or c.S < 2) and share >= 0.5, ("swap", share, n)
        unused = counts == 0
        assert not bool(asc[k][unused].any())
    assert seen > 0 or c.S * per_s < 3


def test_patchify_cls_mean_and_gelu_inputs():
    for shape in mc.PATCHIFY_SHAPES:
        assert lossless_in_16_bit(mc.patchify_image(shape, BF16).to(F64))
        img = mc.patchify_image(shape, F32)
        ref = mc.patchify_ref(img)
        assert torch.equal(ref.to(F32).to(F64), ref) and ref.unique().numel() == img.numel() == ref.numel()
        BT, C, H, W = shape
        # F.unfold's rows against the definition, element by element on the corners of the last patch
        n, gw = (H // 16) * (W // 16), W // 16
        row = BT * n - 1
        ph, pw = (n - 1) // gw, (n - 1) % gw
        for (ch, i, j) in ((0, 0, 0), (C - 1, 15, 15), (C - 1, 0, 15)):
            assert float(ref[row, ch * 256 + i * 16 + j]) == float(img[BT - 1, ch, ph * 16 + i, pw * 16 + j])
    for B, T in mc.CLS_MEAN_CASES:
        rows = ints((B, D), gen("cls_mean", B, T), -64, 64)
        ref = mc.cls_mean_ref(rows, T)
        assert ref.shape == (B * T, D) and torch.equal(ref[::T], ref[T - 1::T])
        if T & (T - 1) == 0:
            assert torch.equal(ref.to(F64), (rows / T).repeat_interleave(T, 0))
    assert any(T & (T - 1) for _, T in mc.CLS_MEAN_CASES)
    assert all(n % 8 == 0 for n, _ in mc.GELU_CASES)
    for dt in mc.DTS:      # one chunk, and a second trip round the grid-stride loop, for every dtype
        chunk = 4 if dt == F32 else 8
        assert {8, mc.GELU_GRID_CHUNKS * chunk + 8} <= {n for n, d in mc.GELU_CASES if d == dt}


# ------------------------------------------------------------------------------------------------ the reference's row maps are the model's rearranges
@pytest.mark.parametrize("dims", mc.GC_DIMS)
def test_row_maps_agree_with_the_models_rearranges(dims):
    """Row ids gathered through the reshape / permute expressions of the divided space-time block (vit.py's header: 'b (n t) m -> (b n) t m',
    the frame batch '(b t) (1 + n) m' with the clip's [CLS] copied to every frame, and the patch embedding's '(b t) n m -> b (n t) m')."""
    B, T, N = dims
    S = 1 + N * T
    ids = torch.arange(B * S).view(B, S, 1)
    tokens = ids[:, 1:]
    skip = tokens.reshape(B, N, T, 1).reshape(B * N, T, 1).reshape(-1)
    assert torch.equal(mc.map_src_rows(MAP_SKIP_CLS, dims, B * N * T)[0], skip)
    xs = tokens.reshape(B, N, T, 1).permute(0, 2, 1, 3).reshape(B * T, N, 1)
    cls = ids[:, :1].unsqueeze(1).expand(B, T, 1, 1).reshape(B * T, 1, 1)
    frame = torch.cat([cls, xs], 1).reshape(-1)
    rows, is_cls = mc.map_src_rows(MAP_FRAME_TOKENS, dims, B * T * (N + 1))
    assert torch.equal(rows, frame) and torch.equal(is_cls.view(B * T, N + 1)[:, 0], torch.ones(B * T, dtype=torch.bool)) and int(is_cls.sum()) == B * T
    # patch embedding: the GEMM rows are (b t) n; written to token rows b (n t) behind [CLS] -- gathering token ids in GEMM-row order inverts that
    embedded = torch.arange(B * T * N).view(B, T, N, 1).permute(0, 2, 1, 3).reshape(B, N * T)
    placed = torch.full((B * S,), -1)
    placed.view(B, S)[:, 1:] = embedded
    rows, _ = mc.map_src_rows(MAP_PATCH_EMBED, dims, B * T * N)
    assert torch.equal(placed[rows], torch.arange(B * T * N))


# ------------------------------------------------------------------------------------------------ planted faults
def _gc_case(mode, dims, rows, **kw):
    return next(c for c in mc.GATHER_CAST_CASES if c.mode == mode and c.dims == dims and c.rows == rows and all(getattr(c, k) == v for k, v in kw.items()))


def test_planted_faults_are_rejected():
    same = mc.same
    # 1. an off-by-one source row in one map
    for mode in (MAP_SKIP_CLS, MAP_FRAME_TOKENS, MAP_PATCH_EMBED):
        c = _gc_case(mode, (2, 4, 9), mc.gc_rows(mode, (2, 4, 9)), dt=BF16)
        x = mc.gc_build(c)
        assert same(mc.gc_expected(c, x), mc.gc_expected(c, x)) and not same(mc.gc_expected(c, x, "src_row_off_by_one"), mc.gc_expected(c, x))
    # 2. a dropped last row when the row count is odd
    c = _gc_case(MAP_IDENTITY, None, 8191, dt=F16)
    x = mc.gc_build(c)
    assert c.rows % 2 == 1 and not same(mc.gc_expected(c, x, "last_row_dropped"), mc.gc_expected(c, x))
    # 3. an unzeroed pad column; 7. one overwritten guard element (every family's buffer)
    for c in (mc.TrCase(1, 200, 256, F32, BF16, False), mc.TrCase(65, 63, 128, F32, F32, True)):
        t = mc.transpose_inputs(c)
        Rp = mc.rpad(c.R, c.pad_to)
        good = mc.transpose_expected(t["x"], Rp, c.dout)
        assert same(good, mc.transpose_expected(t["x"], Rp, c.dout))
        assert not same(mc.transpose_expected(t["x"], Rp, c.dout, fault="unzeroed_pad_column"), good)
        assert not same(mc.transpose_expected(t["x"], Rp, c.dout, fault="guard_overwritten"), good)
        minus = good.clone()
        minus[G:G + c.C, c.R:Rp] = -0.0
        assert mc.pad_is_plus_zero(good, c.C, c.R, Rp) and not mc.pad_is_plus_zero(minus, c.C, c.R, Rp)
    c = _gc_case(MAP_FRAME_TOKENS, (3, 8, 5), mc.gc_rows(MAP_FRAME_TOKENS, (3, 8, 5)), dt=F32)
    assert not same(mc.gc_expected(c, mc.gc_build(c), "guard_overwritten"), mc.gc_expected(c, mc.gc_build(c)))
    # 4. a skipped row that still contributes; 5. a run that absorbs the first row of the next destination
    for kind in ("exact", "order"):
        for pattern in ("mix", "skip_min"):
            c = mc.ScCase(4096, 7, pattern, kind)
            x = mc.sc_build(c)
            touched, good = mc.sc_expected_rows(x, c.V, kind)
            want = mc.table_expected(c.V, touched, good)
            assert same(mc.table_expected(c.V, touched, good), want)
            t4, v4 = mc.sc_expected_rows(x, c.V, kind, fault="skipped_row_contributes")
            assert not same(mc.table_expected(c.V, t4, v4), want)
            t5, v5 = mc.sc_expected_rows(x, c.V, kind, fault="run_absorbs_next")
            assert torch.equal(t5, touched) and not same(mc.table_expected(c.V, t5, v5), want)
            assert not same(mc.table_expected(c.V, touched, good, fault="guard_overwritten"), want)
    # 6. d_t added before d32
    c = next(c for c in mc.GATHER_SEQ_CASES if c.S == 11 and c.pattern == "some_unused" and c.dt == BF16)
    x = mc.gs_build(c)
    for a, b in zip(mc.gs_backward_emulated(c, x), mc.gs_backward_emulated(c, x, swap=True)):
        assert same(a, a.clone()) and not same(b, a)


def test_emulator_adds_in_the_stated_order():
    """2^24 + 1 + 1 in fp32: ascending (big first) loses both ones, descending keeps them."""
    src = torch.tensor([[2.0 ** 24], [1.0], [1.0], [5.0]])
    dest = torch.tensor([0, 0, 0, 1])
    assert mc.emulate_runs(src, dest, 3, "asc").view(-1).tolist() == [2.0 ** 24, 5.0, 0.0]
    assert mc.emulate_runs(src, dest, 3, "desc").view(-1).tolist() == [2.0 ** 24 + 2, 5.0, 0.0]
    assert float(mc.emulate_runs(src, dest, 3, "random", gen("e"))[0]) in (2.0 ** 24, 2.0 ** 24 + 2)
    # the long-run path (one destination at a time): 2^24 followed by 100 ones stays 2^24; the ones first reach 2^24 + 100
    n = 100
    assert n >= mc.RUN_LONG
    src = torch.cat([torch.tensor([[2.0 ** 24, -3.0]]), torch.ones(n, 2), torch.full((2, 2), 7.0)])
    dest = torch.cat([torch.zeros(n + 1, dtype=torch.int64), torch.tensor([2, 2])])
    assert mc.emulate_runs(src, dest, 3, "asc").tolist() == [[2.0 ** 24, n - 3.0], [0.0, 0.0], [14.0, 14.0]]
    assert mc.emulate_runs(src, dest, 3, "desc").tolist() == [[2.0 ** 24 + n, n - 3.0], [0.0, 0.0], [14.0, 14.0]]
    # both paths agree with a plain loop on wide data
    g = gen("emu")
    src, dest = mc.wide((500, 5), g), torch.randint(0, 4, (500,), generator=g)
    dest[:10] = 4
    plain = torch.zeros(6, 5)
    for i in range(500):
        plain[dest[i]] = plain[dest[i]] + src[i]
    assert torch.equal(mc.emulate_runs(src, dest, 6, "asc"), plain)
