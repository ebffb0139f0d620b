"""CPU self-check of tests/temporal_cases.py: the inputs are exact in all three dtypes and have the score gaps their docstrings promise, the
fault-free fp64 emulation of the 16-bit block-diagonal kernels' roundings stays inside the project's allowances (FWD_TOL; GRAD_TOL with
atol x max(1, max|ref|)) on every case tests/test_hip_temporal_stress.py feeds to the HIP kernels, and each planted fault fails at least one
of those cases -- so the GPU file can see those bugs, and a failure there on the fault-free path is not the reference arithmetic's.

Measured peaks of the fault-free emulation, worst error / allowance over DIAG_CASES x KINDS at H = 12 (printed on every run by
test_emulation_stays_inside_the_allowances, which asserts <= 1.0):
    bf16: forward 0.154 (offset, T=2 x 19), lse 0.004, dQ 0.429 (offset, T=16 x 5), dK 0.088, dV 0.085
    fp16: forward 0.130 (peaked, T=8 x 13), lse 0.004, dQ 0.354 (offset, T=16 x 3), dK 0.068, dV 0.057
(dQ of the offset regime is the largest: dS, rounded to dt, meets the 13.75 in K's first four columns.)
"""
import functools

import torch

from tests import temporal_cases as tc
from tests.test_hip_bwd_ops import GRAD_TOL
from tests.test_hip_ops import FWD_TOL

H = 12
DTS = (torch.bfloat16, torch.float16)


@functools.lru_cache(maxsize=None)
def _case(kind, T, groups, h=H):
    qkv, dout = tc.inputs(kind, T, groups, h, tc.seed_of(kind, T, groups, h))
    return qkv, dout, tc.reference(qkv, dout, T, h)


def test_inputs_are_exact_in_every_dtype():
    for T, groups in tc.DIAG_CASES:
        for kind in tc.KINDS:
            qkv, dout, _ = _case(kind, T, groups, 2)
            assert qkv.shape == (T * groups, 3 * 2 * 64) and dout.shape == (T * groups, 2 * 64) and qkv.dtype == torch.float32
            for dt in (torch.float32,) + DTS:
                assert torch.equal(qkv.to(dt).float(), qkv) and torch.equal(dout.to(dt).float(), dout), (kind, T, groups, dt)
    assert not torch.equal(tc.mixed_groups(8, 5, 2, seed=1), tc.mixed_groups(8, 5, 2, seed=2))


def test_case_lists_reach_what_they_claim():
    for T, groups in tc.DIAG_CASES:
        assert 32 % T == 0 and groups % 2 == 1 and ((T * groups) % 32 != 0) == (T != 32)
    assert sorted({T for T, _ in tc.DIAG_CASES}) == [1, 2, 4, 8, 16, 32]
    T, groups = tc.MANY_UNITS_16
    assert tc.units(T * groups, tc.MANY_H) == 2048 + 52          # fwd16 / bwd16: 512 workgroups x 4 waves, then 52 waves go round again
    T, groups = tc.MANY_UNITS_32
    assert tc.units(T * groups, tc.MANY_H) == 8192 + 16 and (T * groups) % 32 == 24   # fp32 forward: 2048 x 4, and a ragged last unit


def test_cold_and_hot_groups_have_the_claimed_score_gaps():
    """Per 32-row unit and head: a cold group's own scores stay below 8 in magnitude; its queries score exactly 128 against the planted key of a
    late_max / early_max group of the same unit and 45 .. 65 against every key of an offset group; the hot groups' own top score is 128 (late_max,
    early_max) or 85 .. 105 (offset)."""
    h = 2
    for T, groups in tc.DIAG_CASES:
        qkv = _case("mixed", T, groups, h)[0]
        t = qkv.double().view(groups, T, 3, h, 64)
        kinds = [tc.group_kind(g) for g in range(groups)]
        seen = set()
        for g in range(groups):
            own = torch.einsum("qhd,khd->hqk", t[g, :, 0], t[g, :, 1]) * tc.SCALE
            if kinds[g] == "cold":
                assert float(own.abs().max()) < 8.0, (T, g)
            elif kinds[g] in ("late_max", "early_max"):
                j = T - 1 if kinds[g] == "late_max" else 0
                assert (own[:, :, j] == 128.0).all() and (T == 1 or float(own[:, :, [x for x in range(T) if x != j]].abs().max()) < 8.0), (T, g)
            elif kinds[g] == "offset":
                assert 85.0 < float(own.min()) and float(own.max()) < 105.0, (T, g)
            for g2 in range(g * T // 32 * 32 // T, min(groups, (g * T // 32 + 1) * 32 // T)):   # the groups of g's unit
                if kinds[g] != "cold" or kinds[g2] in ("cold", "peaked"):
                    continue
                cross = torch.einsum("qhd,khd->hqk", t[g, :, 0], t[g2, :, 1]) * tc.SCALE
                if kinds[g2] == "offset":
                    assert 45.0 < float(cross.min()) and float(cross.max()) < 65.0, (T, g, g2)
                else:
                    assert (cross[:, :, T - 1 if kinds[g2] == "late_max" else 0] == 128.0).all(), (T, g, g2)
                seen.add(kinds[g2])
        if T < 32:
            assert seen, "T=%d groups=%d: no cold group shares a unit with a hot one" % (T, groups)
        else:
            assert not seen


def _emu_ratios(kind, T, groups, dt, ffault=None, bfault=None, h=H):
    """-> [out, lse, dQ, dK, dV] worst error / allowance of the emulation against fp64."""
    qkv, dout, ref = _case(kind, T, groups, h)
    out, lse = tc.emu_fwd(qkv, T, h, dt, ffault)
    res = [tc.excess(out, ref["out"], *FWD_TOL[dt]), tc.excess(lse, ref["lse"], 1e-5, 1e-4)]
    lse_in = lse if torch.isfinite(lse).all() else ref["lse"]
    return res + tc.grad_excess(tc.emu_bwd(qkv, dout, lse_in, T, h, dt, fault=bfault), ref["grad"], *GRAD_TOL[dt])


def test_emulation_stays_inside_the_allowances():
    for dt in DTS:
        peak, where = [0.0] * 5, [None] * 5
        for T, groups in tc.DIAG_CASES:
            for kind in tc.KINDS:
                r = _emu_ratios(kind, T, groups, dt)
                for i in range(5):
                    if r[i] > peak[i]:
                        peak[i], where[i] = r[i], (kind, T, groups)
        print("%s: peaks of error / allowance out %.3f lse %.3f dQ %.3f dK %.3f dV %.3f at %s" % ((dt,) + tuple(peak) + (where,)))
        assert max(peak) <= 1.0, (dt, peak, where)


def test_planted_faults_fail_at_least_one_case():
    caught = {}
    for f in ("no_mask", "tile_max", "pad_last_k"):
        caught["fwd " + f] = max(_emu_ratios(kind, T, groups, dt, ffault=f)[0] for T, groups in tc.DIAG_CASES for kind in ("mixed", "late_max") for dt in DTS)
    for f in tc.BWD_FAULTS:
        caught["bwd " + f] = max(max(_emu_ratios(kind, T, groups, dt, bfault=f)[2:]) for T, groups in tc.DIAG_CASES for kind in ("mixed", "late_max") for dt in DTS)
    # every mixed case with more than one group per unit sees the two mask faults on its own; T = 32 has one group per unit and neither exists
    for T, groups in tc.DIAG_CASES:
        for f in ("no_mask", "tile_max"):
            r = _emu_ratios("mixed", T, groups, torch.bfloat16, ffault=f)[0]
            assert (r > 1.0) == (T < 32), (f, T, groups, r)
    # a K tile left over from the wave's first trip: only a shape beyond 2048 units can see it
    T, groups = tc.MANY_UNITS_16
    qkv, _ = tc.inputs("mixed", T, groups, tc.MANY_H, tc.seed_of("mixed", T, groups))
    ref = tc.reference(qkv, None, T, tc.MANY_H)
    assert tc.excess(tc.emu_fwd(qkv, T, tc.MANY_H, torch.bfloat16)[0], ref["out"], *FWD_TOL[torch.bfloat16]) <= 1.0
    caught["fwd k_unit_minus_2048"] = tc.excess(tc.emu_fwd(qkv, T, tc.MANY_H, torch.bfloat16, "k_unit_minus_2048")[0], ref["out"], *FWD_TOL[torch.bfloat16])
    assert max(_emu_ratios("mixed", 8, 13, torch.bfloat16, ffault="k_unit_minus_2048")) <= 1.0, "39 units cannot see a second trip"
    print("planted faults, worst err / allowed: " + ", ".join("%s %.3g" % kv for kv in caught.items()))
    for f, w in caught.items():
        assert w > 1.0, "planted fault %s passes every case (worst err / allowed %.3g)" % (f, w)
    assert len(caught) == len(tc.FWD_FAULTS) + len(tc.BWD_FAULTS)
