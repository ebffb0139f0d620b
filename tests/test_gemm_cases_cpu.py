"""CPU self-check of tests/gemm_cases.py: the cases test what they claim, so that none can pass vacuously on the GPU
(tests/test_hip_gemm_exact.py), and the comparison used there rejects three planted faults."""
import pytest
import torch

from tests import gemm_cases as gc
from tests.gemm_cases import BF16, F16, F32, F64

CASES = gc.GEMM_CASES
IDS = [c.id for c in CASES]
LIMIT = 2.0 ** 24


def _valid_rows(c, t):
    """Drop what the planted NaN of a nan_row case reaches (identity map: row M - 1)."""
    return t[:c.M - 1] if gc.EPI[c.epi].get("nan_row") else t


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_case_is_exact_in_fp32_in_any_summation_order(c):
    """Products and partial sums stay integers below 2^24 through the largest scale of the epilogue, and an fp32 evaluation with the K
    columns permuted equals the fp64 reference bitwise (the pre-activations only, for the GELU family)."""
    x = gc.build(c)
    scale = max(1.0, float(x.row_scale.max()) if x.row_scale is not None else 1.0) * (1.0 / (1.0 - gc.DROP_P) if x.drop_seed else 1.0)
    if x.act == gc.ACT_MUL_SAVED:
        scale *= float(x.saved.to(F64).abs().max())
    bound = float(_valid_rows(c, x.ref["products"]).max()) * scale + sum(float(t.abs().max()) for t in (x.bias, x.bias2, x.residual) if t is not None)
    assert bound < LIMIT, bound
    assert c.K <= 3072
    perm = torch.randperm(c.K, generator=gc.gen("perm", c.id))
    r32 = gc.reference(x, f=F32, perm=perm)
    keys = ("pre",) if not c.exact else ("pre", "out", "c2", "side")
    for k in keys:
        if x.ref[k] is not None:
            assert r32[k].dtype == F32
            assert torch.equal(_valid_rows(c, r32[k]).to(F64), _valid_rows(c, x.ref[k])), k
    if c.dt == F16 and c.exact:
        assert float(_valid_rows(c, x.ref["out"]).abs().max()) <= 60000.0
        assert x.ref["c2"] is None or float(x.ref["c2"].abs().max()) <= 60000.0


@pytest.mark.parametrize("c", [c for c in CASES if c.exact and c.out_dtype != F32], ids=lambda c: c.id)
def test_sixteen_bit_output_cases_exercise_the_rounding(c):
    """At least 5 % of the reference elements are not representable in the output dtype, and at least one is an exact tie."""
    x = gc.build(c)
    ref = _valid_rows(c, x.ref["out"])
    ref = ref[(ref != gc.SENTINEL).any(1)]
    assert float((~gc.representable(ref, c.out_dtype)).double().mean()) >= 0.05
    assert bool(gc.exact_ties(ref, c.out_dtype).any())


def test_tie_detection_and_ties_to_even():
    assert gc.exact_ties(torch.tensor([257.0, 259.0, 258.0, 256.5, -257.0, 514.0, 515.0], dtype=F64), BF16).tolist() == [True, True, False, False, True, True, False]
    assert torch.tensor([257.0, 259.0, -257.0], dtype=F64).to(BF16).tolist() == [256.0, 260.0, -256.0]
    assert gc.exact_ties(torch.tensor([2049.0, 2050.0, 4098.0, 4097.0], dtype=F64), F16).tolist() == [True, False, True, False]
    assert torch.tensor([2049.0, 2051.0], dtype=F64).to(F16).tolist() == [2048.0, 2052.0]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_epilogue_of_the_case_is_not_trivial(c):
    x = gc.build(c)
    e = gc.EPI[c.epi]
    pre = x.ref["pre"]
    if x.act == gc.ACT_RELU:
        assert float((pre > 0).double().mean()) >= 0.25 and float((pre < 0).double().mean()) >= 0.25
    if x.drop_seed:
        assert gc.DROP_P == 0.5
        assert 0.4 <= float(gc.keep_mask(x.drop_seed, c.M, c.N).mean()) <= 0.6
    if x.row_scale is not None:
        n_groups = (c.M + c.group - 1) // c.group
        assert x.row_scale.numel() == n_groups
        assert set(x.row_scale.tolist()) <= {0.0, 0.5, 1.0, 2.0}
        if n_groups >= 2:     # every group boundary inside [0, M) is crossed by construction: one scale per group, all groups present
            assert all((b * c.group) < c.M for b in range(1, n_groups))
            assert bool((x.row_scale == 0).any()) and bool((x.row_scale != 1).any())
            assert bool((x.row_scale[1:] != x.row_scale[:-1]).all())
        else:
            assert c.M == 1 and c.map_dims == (1, 1, 1)      # (a single row has a single group; nothing else may)
    if e.get("inexact"):
        assert float(pre.abs().max()) <= 6.0 and float((pre.abs() <= 3.0).double().mean()) >= 0.5
        assert x.alpha == 2.0 ** round(torch.log2(torch.tensor(x.alpha)).item())
        if x.saved is not None:
            assert float(x.saved.to(F64).abs().max()) <= 6.0
    if x.act == gc.ACT_MUL_SAVED:
        assert torch.equal(x.saved.to(F64), x.saved.to(F64).round()) and bool((x.saved.to(F64).abs() > 1).any())
    if e.get("nan_row"):
        a = x.a.to(F64)
        assert int(a.isnan().sum()) == 1 and bool(a[c.M - 1].isnan().any())
        assert bool(x.ref["out"][c.M - 1].isnan().all()) and not bool(x.ref["out"][:c.M - 1].isnan().any())
    if x.map_mode != gc.MAP_IDENTITY:
        hit = torch.zeros(x.out_rows, dtype=torch.bool)
        hit[x.orow[~x.is_side]] = True
        assert int(hit.sum()) == int((~x.is_side).sum())                # the map is injective ...
        assert not bool(hit[::1 + c.map_dims[2] * c.map_dims[1]].any())     # ... and never reaches a CLS row
        assert int(x.is_side.sum()) == x.side_rows


def _cells():
    """What the table covers, as sets of cells."""
    s = set()
    for c in CASES:
        s.add(("shape", c.route, gc.DT_NAME[c.dt], c.M, c.N, c.K))
        s.add(("epi", c.route, gc.DT_NAME[c.dt], c.out, c.epi, c.group, c.map_dims, c.tiled))
        s.add(("layout", c.route, gc.DT_NAME[c.dt], c.layout, "res" if gc.EPI[c.epi].get("res") else c.epi))
        for v in c.variants:
            s.add(("opts", c.route, gc.DT_NAME[c.dt], c.epi, v))
    return s


def test_the_table_covers_every_cell():
    """Every cell of the issue's case list, spelled out here independently of the table's construction: deleting a case fails this."""
    have = _cells()
    want = set()
    o = lambda *p: tuple(zip(p[::2], p[1::2]))   # noqa: E731
    k128, p256, q8, q8g = o("gemm_tile", 128), o("gemm_tile", 256, "gemm_kind", 0), o("gemm_tile", 256, "gemm_kind", 1), o("gemm_tile", 256, "gemm_kind", 1, "gemm_grid", 8)
    exact_epis = ("plain", "bias_alpha", "relu_copy", "mul_saved", "gelu", "gelu_save", "gelu_bwd", "dropout")
    for dt in ("f32", "bf16", "f16"):
        k1 = 32 if dt == "f32" else 64
        outs = ("f32",) if dt == "f32" else ("same", "f32")
        want |= {("shape", "k128", dt, M, N, 2 * k1) for M in (1, 127, 128, 129, 257) for N in (2, 8, 100, 128, 132, 260)}
        want |= {("shape", "k128", dt, 129, 100, K) for K in (k1, 2 * k1, 3 * k1, 768)}
        want |= {("shape", "p256", dt, M, N, 128) for M in (1, 255, 256, 257, 384, 513) for N in (8, 256, 264, 520)}
        want |= {("shape", "p256", dt, 257, 264, K) for K in (128, 192, 768)}
        want.add(("shape", "p256", dt, 11 * 256 - 100, 256, 128))
        for route, opts in (("k128", k128), ("p256", p256)):
            for out in outs:
                want |= {("epi", route, dt, out, e, 0, None, False) for e in exact_epis}
                want |= {("epi", route, dt, out, "res_scale", g, None, False) for g in (1, 7, 65)}
                want |= {("epi", route, dt, out, e, 0, dims, False) for e in ("skip_cls", "frame", "patch") for dims in ((2, 4, 9), (1, 1, 1))}
                want |= {("epi", route, dt, out, "skip_cls_bias2", 5, dims, False) for dims in ((2, 4, 9), (1, 1, 1))}
            want |= {("layout", route, dt, lay, e) for lay in ("wide_in", "wide_out", "row1") for e in ("plain", "res")}
            want.add(("layout", route, dt, "tight", "nan_row"))
            want |= {("opts", route, dt, e, opts) for e in exact_epis}
        want |= {("opts", "p256", dt, e, p256 + o("gemm_grid", 8) + tail) for e in ("bias", "res_scale", "gelu_save") for tail in ((), o("gemm_tail", 0))}
    want |= {("opts", "p256", "bf16", "plain", p256 + t) for t in ((), o("gemm_tune", 0), o("gemm_tune", 2))}
    for dt in ("bf16", "f16"):
        rt = lambda M: "q8" if M % 16 == 0 else "q8_rem"   # noqa: E731
        want |= {("shape", rt(M), dt, M, N, 256) for M in (256, 512, 528, 752, 520, 612) for N in (256, 512)}
        want |= {("shape", rt(M), dt, M, N, K) for (M, N) in ((528, 256), (612, 512)) for K in (256, 384, 768)}
        want.add(("shape", "q8_tail", dt, 10 * 256 + 64, 256, 2048))
        for route in ("q8", "q8_rem"):
            want |= {("epi", route, dt, "same", e, 0, None, False) for e in ("plain", "bias", "relu", "mul_saved", "gelu_save", "gelu", "dropout")}
            want |= {("epi", route, dt, "same", "scale", g, None, False) for g in (8, 9, 16, 197)}
            want |= {("epi", route, dt, "f32", "res_scale", g, None, False) for g in (16, 17)}
            want |= {("epi", route, dt, "same", "scale_drop", g, None, False) for g in (9, 197)}         # split launches: a group that straddles the split, and dropout
            want |= {("opts", route, dt, "plain", q8 + v) for v in ((), o("gemm_sched", 0), o("gemm_epi", 0), o("gemm_grid", 8), o("cu_budget", 64))}
            want.add(("layout", route, dt, "tight", "nan_row"))
        want |= {("epi", "q8", dt, "same", e, 0, None, True) for e in ("mul_saved", "gelu_save")}
        want |= {("epi", "p256", dt, "same", "scale", 7, None, False), ("epi", "p256", dt, "f32", "res_scale", 15, None, False)}
        want |= {("opts", "p256", dt, "scale", q8), ("opts", "p256", dt, "res_scale", q8), ("opts", "p256", dt, "bias", q8)}
        want |= {("epi", "q8_tail", dt, "f32", "res_scale", 1569, None, False), ("epi", "q8_tail", dt, "same", "bias", 0, None, False), ("epi", "q8_tail", dt, "same", "scale_drop", 1569, None, False)}
        want |= {("opts", "q8_tail", dt, e, q8g + tail) for e in ("bias", "res_scale") for tail in ((), o("gemm_tail", 0))}
        want |= {("layout", "p256", dt, lay, "bias") for lay in ("lda8", "lda8_row1")}
        want |= {("shape", "p256", dt, 528, 256, 192), ("shape", "p256", dt, 528, 264, 256)}
        want |= {("layout", "q8", dt, lay, e) for lay in ("wide_in", "wide_out", "row1") for e in ("plain", "res")}
    assert want <= have, sorted(map(str, want - have))[:20]
    assert len(CASES) == len(set(IDS))
    # the other tables, literally
    assert gc.BATCH_JOBS == ((1, 8, 64, "bias", "same"), (130, 200, 128, "bias_alpha", "f32"), (128, 128, 768, "res", "f32"), (257, 132, 64, "plain", "same"), (768, 768, 768, "bias_alpha", "same"))
    assert {gc.EPI[j[3]].get(k, False) for j in gc.BATCH_JOBS for k in ("bias", "alpha", "res")} >= {True, 0.5} and any(j[4] == "f32" for j in gc.BATCH_JOBS)
    assert set(gc.TN_SHAPES) >= {(M, N, K) for M in (1, 31, 32, 33, 130, 1000) for N in (8, 256, 264, 520) for K in (8, 256, 264)}
    assert gc.TN_SPLITS == (0, 1, 2, 3, 7, 64) and (130 + 31) // 32 < 64


def test_split_cases_put_the_second_launch_inside_a_row_scale_group():
    """Split launches: the first row of the second launch lies strictly inside a row-scale group whose neighbours carry other scales, so a scale or a
    dropout index taken relative to the launch's own first row cannot give the reference's bits."""
    n = 0
    for c in CASES:
        if c.split_row is None or not gc.EPI[c.epi].get("scale") or c.split_row % c.group == 0:
            continue
        x = gc.build(c)
        gi = c.split_row // c.group
        assert gi * c.group < c.split_row < min((gi + 1) * c.group, c.M)
        assert gi == 0 or float(x.row_scale[gi - 1]) != float(x.row_scale[gi])
        shifted = x.row_scale[(torch.arange(c.split_row, c.M) - c.split_row) // c.group]
        assert not torch.equal(shifted, x.row_scale[torch.arange(c.split_row, c.M) // c.group])
        n += 1
    assert n >= 8


# ------------------------------------------------------------------------------------------------ sharpness: planted faults
def _first(pred):
    return [c for c in CASES if pred(c)]


@pytest.mark.parametrize("fault,pred", [
    ("scale_row_off_by_one", lambda c: gc.EPI[c.epi].get("scale") and c.exact and not c.map_dims and c.M > 1),
    ("bias_after_rounding", lambda c: gc.EPI[c.epi].get("bias") and c.exact and c.out_dtype != F32 and not gc.EPI[c.epi].get("nan_row")),
    ("dropout_without_m_off", lambda c: gc.EPI[c.epi].get("drop") and c.split_row is not None),
])
def test_the_comparison_rejects_a_planted_fault(fault, pred):
    """The GPU test's comparison (gemm_cases.matches: the fp64 reference rounded once, torch.equal) accepts the reference evaluated in fp32 and
    rejects it with one fault planted -- in EVERY case the fault applies to."""
    cases = _first(pred)
    assert len(cases) >= 4, fault
    for c in cases:
        x = gc.build(c)
        good = gc.reference(x, f=F32)["out"].to(c.out_dtype)
        assert gc.matches(good, x.ref["out"], c.out_dtype), c.id
        bad = gc.reference(x, fault=fault)["out"].to(c.out_dtype)
        assert not gc.matches(bad, x.ref["out"], c.out_dtype), (fault, c.id)


# ------------------------------------------------------------------------------------------------ weight-gradient cases
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_weight_gradient_cases_are_exact(dt):
    for (M, N, K) in gc.TN_SHAPES:
        t = gc.tn_inputs(M, N, K, dt)
        assert float(t["products"].max()) + 100 < LIMIT
        perm = torch.randperm(M, generator=gc.gen("perm", M, N, K))
        c32 = t["c0"] + t["a"].float()[perm].T @ t["b"].float()[perm]
        assert torch.equal(c32.to(F64), t["ref_c"])
        assert torch.equal((t["cs0"] + t["a"].float()[perm].sum(0)).to(F64), t["ref_cs"])
        assert bool((t["ref_c"] != t["c0"].to(F64)).any())


def test_poisoned_views():
    t = torch.arange(12.0).view(3, 4)
    v = gc.poisoned(t, 2, 3, 1)
    assert torch.equal(v, t) and v._base.shape == (6, 7) and v.stride() == (7, 1) and v.storage_offset() == 7
    assert int(v._base.isnan().sum()) == 6 * 7 - 12
    o = gc.poisoned(t.to(BF16), gc.GUARD_ROWS, 0, 0, fill=gc.SENTINEL)
    assert o._base.shape == (3 + 256, 4) and bool((o._base[3:] == gc.SENTINEL).all())
    b = gc.poisoned_vec(torch.ones(5), 3)
    assert b.numel() == 5 and int(b._base.isnan().sum()) == 3
