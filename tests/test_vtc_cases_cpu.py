"""CPU self-check of tests/vtc_cases.py: the cases' dot products are exact in fp32 and their fp64 references finite, the regimes have the
properties their names promise, the fault-free fp32 emulator of the five contrastive-loss kernels stays within a quarter of every recorded
allowance constant against fp64 (that is where the constants come from), every planted fault exceeds the allowance of a named output on a
named case, and on benign inputs the allowances stay tight -- so what tests/test_hip_vtc_stress.py holds the HIP kernels to can see those
bugs and is not fitted to the kernels."""
import functools

import pytest
import torch

from tests import vtc_cases as vc

F32, F64 = torch.float32, torch.float64
GRADS = ("dv", "dt", "dgv", "dgt", "dtemp")


@functools.lru_cache(maxsize=None)
def _sweep():
    """One pass over every case (dloss = 1.7; gauss also loss-scaled): reference, allowances and the fault-free emulator, once for all tests.
    -> list of dicts(case name, shape, regime, temp, dloss, exact, finite, ratios {output: error / A}, tight {gradient: max A / max |ref|},
    emu_rel {gradient: max emulator error / max |ref|})."""
    rows = []
    for c in vc.cases():
        sv, st = c.v @ c.gt.t(), c.t @ c.gv.t()
        exact = (torch.equal(sv.double(), c.v.double() @ c.gt.double().t()) and torch.equal(st.double(), c.t.double() @ c.gv.double().t())
                 and all(torch.equal(torch.round(x.double() / vc.STEP) * vc.STEP, x.double()) for x in (c.v, c.t, c.gv, c.gt)))
        for dl in ((1.7, vc.SCALED_DLOSS) if c.regime == "gauss" and float(c.temp) in [float(torch.tensor(t, dtype=F32)) for t in vc.SCALED_TEMPS] else (1.7,)):
            ds64 = {}
            ref, A, got = vc.reference(c, dl), vc.allowances(c, dl, ds64), vc.emu(c, dl)
            ref.update(ds64)
            top = {k: float(ref[k].abs().max()) for k in GRADS}
            rows.append(dict(name=c.name, shape=(c.B, c.G, c.E, c.col0), regime=c.regime, temp=float(c.temp), dloss=dl, exact=exact,
                             finite=all(bool(torch.isfinite(ref[k]).all()) for k in vc.OUTPUTS + vc.SAVED),
                             ratios={k: w for k, (w, _) in vc.ratios(got, ref, A).items()},
                             tight={k: float(torch.as_tensor(A[k]).max()) / top[k] if top[k] > 0 else 0.0 for k in GRADS},
                             emu_rel={k: float((got[k].double() - ref[k]).abs().max()) / top[k] if top[k] > 0 else 0.0 for k in GRADS},
                             zero=all(float(got[k].abs().max()) == 0 and float(ref[k].abs().max()) == 0 for k in ("loss",) + GRADS)))
    return rows


def test_dot_products_are_exact_in_fp32_and_references_finite():
    rows = _sweep()
    assert len(rows) == len(vc.SHAPES) * (len(vc.REGIMES) * len(vc.TEMPS) + len(vc.SCALED_TEMPS))
    for r in rows:
        assert r["exact"], "%s: a q . k sum is not exact in fp32, or a row is off the 2^-10 grid" % r["name"]
        assert r["finite"], "%s: the fp64 reference is not finite" % r["name"]
        if r["shape"][:2] == (1, 1):      # one pair: the loss is lse - sim = 0 and every gradient 0, in fp32 and in fp64 alike
            assert r["zero"], r["name"]


def test_emulator_stays_within_a_quarter_of_every_constant():
    """Re-measures vc.MEASURED: the worst error / A of the fault-free emulator per family of outputs.  Above C / 4 the margin is gone; below
    C / 8 the recorded constant is stale (the derivation or the cases changed) and has to be measured again."""
    worst = {}
    for r in _sweep():
        for k, w in r["ratios"].items():
            f = vc.FAMILY[k]
            if w > worst.get(f, (-1.0, ""))[0]:
                worst[f] = (w, "%s %s dloss %g" % (r["name"], k, r["dloss"]))
    print()
    for f, (w, where) in worst.items():
        print("[vtc allowance] %-5s emulator / A %.4f (recorded %.4f, constant %.2f) at %s" % (f, w, vc.MEASURED[f], vc.C[f], where))
    for r in _sweep():
        if r["regime"].startswith("offset") and abs(r["temp"] - 0.001) < 1e-9 and r["shape"][1] > 1:
            print("[vtc conditioning] %s: d temp of the emulator is %.2g of its value off, allowance %.2g of it" % (
                r["name"], r["emu_rel"]["dtemp"], vc.C["dtemp"] * r["tight"]["dtemp"]))
    assert set(worst) == set(vc.C)
    for f, (w, where) in worst.items():
        assert vc.C[f] == vc.MARGIN * vc.RECORDED[f] and vc.MEASURED[f] <= vc.RECORDED[f]
        assert w <= vc.C[f] / 4, "%s: emulator at %.3f x A (%s), the constant %.3f leaves less than the margin of 4" % (f, w, where, vc.C[f])
        assert w >= vc.C[f] / 8, "%s: emulator at most %.3f x A, the constant %.3f is stale" % (f, w, vc.C[f])


# fault -> (shape, regime, temp, the output whose allowance it exceeds there)
FAULT_CASES = {
    "no_max": ((3, 3, 256, 0), "offset_pos", 0.001, "lse"),                     # exp(1000) overflows
    "max_first256": ((64, 512, 256, 448), "late_neg_last", 0.001, "lse"),        # column 511 is 880 above the first 256
    "pos_at_i": ((5, 13, 12, 8), "gauss", 0.07, "loss"),
    "no_clamp": ((3, 3, 256, 0), "gauss", 0.9, "sim_v2t"),
    "inv_b": ((3, 3, 256, 0), "gauss", 0.07, "loss"),
    "dtemp_one_dir": ((3, 3, 256, 0), "gauss", 0.07, "dtemp"),
    "swap_dg": ((5, 13, 4, 3), "gauss", 0.07, "dgv"),
    "loss_first256": ((130, 260, 64, 130), "gauss", 0.07, "loss"),
    "dq_no_tc": ((7, 21, 1024, 0), "gauss", 0.07, "dv"),
}
# the same faults where the conditioning terms are at their widest: a second case each, so that no allowance hides them there
FAULT_CASES_HARD = {
    "no_clamp": ((5, 13, 4, 3), "offset_neg", 0.0001, "dtemp"),
    "pos_at_i": ((16, 8192, 32, 8176), "dup", 0.01, "dv"),
    "dtemp_one_dir": ((130, 260, 64, 130), "offset_pos", 0.001, "dtemp"),
    "dq_no_tc": ((5, 13, 12, 8), "aligned", 0.5, "dt"),
    "max_first256": ((130, 260, 64, 130), "late_neg_last", 0.01, "lse"),
}


@pytest.mark.parametrize("table", [FAULT_CASES, FAULT_CASES_HARD], ids=["plain", "hard"])
def test_every_planted_fault_exceeds_an_allowance(table):
    if table is FAULT_CASES:
        assert set(table) == set(vc.FAULTS)
    for fault, (shape, regime, temp, out) in table.items():
        c = vc.build(shape, regime, temp)
        ref, A = vc.reference(c, 1.7), vc.allowances(c, 1.7)
        clean = vc.ratios(vc.emu(c, 1.7), ref, A)
        assert all(w <= vc.C[vc.FAMILY[k]] / 4 for k, (w, _) in clean.items()), (fault, clean)
        bad = vc.ratios(vc.emu(c, 1.7, fault=fault), ref, A)
        print("[vtc fault] %-14s on %s: %s at %.3g x A (constant %.2f)" % (fault, c.name, out, bad[out][0], vc.C[vc.FAMILY[out]]))
        assert bad[out][0] > vc.C[vc.FAMILY[out]], "%s passes on %s: %s at %.3g x A" % (fault, c.name, out, bad[out][0])
        with pytest.raises(AssertionError, match=c.name.replace("+", r"\+").replace(".", r"\.")):
            vc.check(c, vc.emu(c, 1.7, fault=fault), ref, A)


def test_allowances_stay_tight_where_the_problem_is_benign():
    """gauss at temp = 0.07: the allowance of each gradient and of d temp is at most 1e-4 of the output's largest reference magnitude (the
    one-pair shape aside: its outputs are exactly 0 and are held to exactly 0)."""
    n = 0
    for r in _sweep():
        if r["regime"] == "gauss" and abs(r["temp"] - 0.07) < 1e-6 and r["shape"][:2] != (1, 1):
            n += 1
            for k in GRADS:
                allowed = vc.C[vc.FAMILY[k]] * r["tight"][k]
                assert allowed <= 1e-4, "%s dloss %g: the allowance of %s is %.2e of its largest magnitude" % (r["name"], r["dloss"], k, allowed)
                assert r["emu_rel"][k] <= 2e-6, (r["name"], k, r["emu_rel"][k])
    assert n == 2 * (len(vc.SHAPES) - 1)


def test_regimes_do_what_they_claim():
    for shape in vc.SHAPES:
        B, G, E, col0 = shape
        pos = torch.arange(B)
        for regime in vc.REGIMES:
            c = vc.build(shape, regime, 0.01)
            assert c.v.shape == (B, E) and c.gv.shape == (G, E) and c.gt.shape == (G, E) and c.temp.dtype == F32 and c.v.dtype == F32
            assert torch.equal(c.v, c.gv[col0:col0 + B]) and torch.equal(c.t, c.gt[col0:col0 + B])
            assert all(x.is_contiguous() for x in (c.v, c.t, c.gv, c.gt))
            tc = float(vc.clamped(c.temp))
            sims = (c.v.double() @ c.gt.double().t() / tc, c.t.double() @ c.gv.double().t() / tc)
            for sim in sims:
                if regime in ("late_neg_last", "late_neg_first"):
                    col = vc.late_col(regime, G)
                    assert col == (G - 1 if regime == "late_neg_last" else 0) and (regime != "late_neg_last" or G <= 256 or col >= 256)
                    rows = pos[col0 + pos != col]          # (in the row whose positive that column is there is nothing to beat)
                    if len(rows):
                        assert (sim[rows].argmax(1) == col).all()
                        assert float((sim[rows, col] - sim[rows, col0 + rows]).min()) >= 0.8 / tc
                if regime == "offset_pos":
                    assert float((sim * tc - 1).abs().max()) <= 0.02
                if regime == "offset_neg":
                    assert float((sim * tc + 1).abs().max()) <= 0.02
                if regime == "aligned":
                    assert (sim.argmax(1) == col0 + pos).all()
            if regime == "aligned":
                assert float((c.gv - c.gt).abs().max()) <= 2 * vc.STEP and (G * E < 64 or not torch.equal(c.gv, c.gt))
            if regime == "dup":
                for x in (c.gv, c.gt):
                    assert (x[0::3] == x[0]).all() and (G < 3 or not torch.equal(x[1], x[0]))
                inside = [j for j in range(col0, col0 + B) if j % 3 == 0]
                assert G < 9 or (len(inside) >= 1 and 0 < len(range(0, G, 3)) - len(inside))     # copies inside and outside the own block
                for sim in sims:                                     # exact ties; a positive among the copies ties with every copy
                    assert (sim[:, 0::3] == sim[:, :1]).all()
                    for j in inside:
                        assert int((sim[j - col0] == sim[j - col0, j]).sum()) >= len(range(0, G, 3))
    assert not torch.equal(vc.build(vc.SHAPES[1], "gauss", 0.07, seed=1).gv, vc.build(vc.SHAPES[1], "gauss", 0.07).gv)
    assert [float(vc.clamped(torch.tensor(t))) for t in (0.0001, 0.9)] == [float(torch.tensor(0.001, dtype=F32)), 0.5]
