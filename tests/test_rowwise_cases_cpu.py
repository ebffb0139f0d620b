"""CPU self-check of tests/rowwise_cases.py: the stress regimes have the properties their names promise, the fault-free fp32 emulators of
the row-wise kernels stay inside every allowance against fp64 (that is where the allowance constants come from), and each planted fault
fails at least one case -- so the cases tests/test_hip_rowwise_stress.py feeds to the HIP kernels can see those bugs."""
import math

import torch

from tests import rowwise_cases as rc

F32, F64 = torch.float32, torch.float64
FWD32 = (1e-5, 1e-5)            # the project's fp32 LayerNorm pair
BWD_DX, BWD_DG = (1e-4, 2e-4), (1e-4, 2e-3)


def _pow2_at_least(r):
    return 2.0 ** math.ceil(math.log2(max(r, 1e-30)))


def test_rowwise_regimes_do_what_they_claim():
    for regime in rc.LN_REGIMES:
        x = rc.ln_rows(105, regime, seed=3)
        assert x.dtype == F32 and x.shape == (105, 768) and torch.isfinite(x).all()
        assert torch.equal(x.double().float(), x)
        assert not torch.equal(rc.ln_rows(105, regime, seed=4), x)
    x = rc.ln_rows(105, "gauss", 0).double()
    assert 2.2 < float(x.std(-1).mean()) < 2.8 and 0.2 < float(x.mean()) < 0.6
    x = rc.ln_rows(105, "offset", 0).double()
    ratio = x.mean(-1).abs() / x.std(-1)
    assert float(ratio.min()) >= 50 and 50 <= float(x.mean(-1).abs().min()) and float(x.mean(-1).abs().max()) <= 205
    assert (x.mean(-1) > 0).any() and (x.mean(-1) < 0).any() and 0.08 < float(x.std(-1).min()) and float(x.std(-1).max()) < 1.1
    x = rc.ln_rows(105, "outlier", 0).double()
    for r in range(105):
        cols = rc.OUTLIER_COLS[:2 + r % 5]
        big = (x[r].abs() >= 59).nonzero().flatten().tolist()
        assert sorted(big) == sorted(cols) and float(x[r].abs().max()) <= 201, r
    assert rc.OUTLIER_COLS[0] == 767 and rc.OUTLIER_COLS[1] < 4 and rc.OUTLIER_COLS[2] >= 512 and 4 <= rc.OUTLIER_COLS[2] % 256 < 252
    x = rc.ln_rows(105, "scale_span", 0).double()
    sd = x.std(-1)
    assert float(sd.max() / sd.min()) > 2.0 ** 19 and float(sd.min()) < 2.6 * 2.0 ** -10 * 1.2
    x = rc.ln_rows(105, "flat", 0).double()
    const = torch.arange(105) % 4 == 1
    assert (x[const].std(-1) == 0).all() and (x[~const].std(-1) > 0).all()
    assert float(x[~const].std(-1).max()) < 1.2 * 2.0 ** -10 and 0.89 < float(x.mean(-1).min()) and float(x.mean(-1).max()) < 1.11
    x = rc.ln_rows(105, "mixed", 0).double()
    cv = x.std(-1) / x.mean(-1).abs()
    assert (cv[0::5] < 0.02).all() and (cv[1::5] < 0.002).all() and (x[2::5].abs().amax(-1) >= 59).all()   # offset, flat, outlier rows in turn
    for dt in (torch.bfloat16, torch.float16):
        d = rc.delta_rows(40, dt, seed=1)
        assert d.dtype == dt and torch.isfinite(d.float()).all()
    g, b = rc.ln_params(0)
    assert torch.equal(g.double().float(), g) and 0.5 < float(g.min()) and float(b.abs().max()) < 0.5
    # cross-entropy
    for V in rc.XENT_V:
        for M in (1, 83):
            for regime in rc.XENT_REGIMES:
                x, lab = rc.xent_inputs(M, V, regime, seed=1)
                assert x.dtype == F32 and x.shape == (M, V) and lab.dtype == torch.int64 and torch.isfinite(x).all()
                assert int(lab.min()) >= 0 and int(lab.max()) < V and int(lab[0]) == V - 1 and (M == 1 or int(lab[1]) == 0 or regime == "wide")
                xd = x.double()
                if regime == "late_max":
                    assert (xd.argmax(-1) == V - 1).all() and (V < 3 or float((xd[:, V - 1] - xd[:, :V - 1].amax(-1)).min()) >= 99.9)
                if regime == "offset":
                    assert float(xd.min()) > 2.9e4 and float(xd.max()) < 3.1e4
                if regime == "peaked":
                    top2 = xd.topk(2, -1).values
                    assert float((top2[:, 0] - top2[:, 1]).min()) >= 59.9
                    hit = xd.argmax(-1) == lab
                    assert hit[0::2].all() and not hit[1::2].any()
                if regime == "wide":
                    assert float(xd.max()) == 80.0 and float(xd.min()) >= -80.0
                    if M > 2 and V > 2:
                        assert (xd[2::3].gather(1, lab[2::3, None]).squeeze(1) == xd[2::3].amin(-1)).all()
                        assert float((torch.exp(xd - 80.0).float() == 0).double().mean()) > 0.2
    # optimizer
    p, g, m, v = rc.adamw_inputs(100001)
    nz = g != 0
    assert float(g[nz].abs().min()) < 2e-6 and float(g.abs().max()) > 5e2 and float(g.abs().max()) <= 1e3
    assert float(v[nz].min()) < 1e-29 and ((g == 0) == (v == 0)).all() and int((g == 0).sum()) > 9000
    assert math.isfinite(float((g.double() ** 2).sum().float())) and torch.isfinite(g * g).all()
    assert rc.ADAMW_S == 4194304


LN_EMU_SHAPES = (1, 3, 5, 74, 105)


def _ln_emu_ratios(order, fault=None):
    """Worst err / allowed of the forward emulator over every regime; also the raw ratio err / (2^-24 max|x| rstd max|gamma|) beyond the
    plain tolerance (what LN_C is read from)."""
    worst, raw = 0.0, 0.0
    g, b = rc.ln_params(0)
    for regime in rc.LN_REGIMES:
        eps = rc.LN_EPS[regime]
        for rows in LN_EMU_SHAPES:
            x = rc.ln_rows(rows, regime, seed=rows)
            y, mean, rstd = rc.emu_ln(x, g, b, eps, order, fault)
            ry, rm, rr = rc.ln_ref(x, g, b, eps)
            worst = max(worst, rc.excess(y, ry, *FWD32, rc.ln_fwd_extra(x, g, eps)))
            em, er = rc.ln_stats_extra(x, eps)
            worst = max(worst, rc.excess(mean, rm, *FWD32, em), rc.excess(rstd, rr, *FWD32, er))
            if fault is None:
                unit = rc.ln_fwd_extra(x, g, eps, c=1.0)
                over = ((y.double() - ry).abs() - (FWD32[1] + FWD32[0] * ry.abs())).clamp(min=0)
                raw = max(raw, float((over / unit).max()))
    return worst, raw


def _ln_bwd_emu_ratios(order):
    worst, raw = 0.0, 0.0
    g, _ = rc.ln_params(1)
    for regime in rc.LN_REGIMES:
        eps = rc.LN_EPS[regime]
        for rows in (5, 105, 300):
            x = rc.ln_rows(rows, regime, seed=rows + 1)
            dy = rc.delta_rows(rows, F32, seed=rows)
            dx, ag = rc.emu_ln_bwd(x, dy, g, eps, order)
            rdx, rag = rc.ln_bwd_ref(x, dy, g, eps)
            worst = max(worst, rc.excess(dx, rdx, *BWD_DX, rc.ln_dx_extra(x, dy, g, eps)))
            worst = max(worst, rc.excess(ag.sum(0), rag.sum(0), *BWD_DG, rc.ln_dgamma_extra(x, dy, eps)))
            unit = rc.ln_dx_extra(x, dy, g, eps, c=1.0)
            over = ((dx.double() - rdx).abs() - (BWD_DX[1] + BWD_DX[0] * rdx.abs())).clamp(min=0)
            raw = max(raw, float((over / unit).max()))
    return worst, raw


XENT_EMU_CASES = [(M, V) for V in rc.XENT_V for M in (1, 83)]


def _xent_emu_ratios(order, fault=None):
    worst, raw = 0.0, 0.0
    for M, V in XENT_EMU_CASES:
        if order == "seq" and V > 4000:
            continue       # 30522 sequential additions per row: the lane order covers that size
        for regime in rc.XENT_REGIMES:
            x, lab = rc.xent_inputs(M, V, regime, seed=2)
            loss, grad = rc.emu_xent(x, lab, 1.0 / M, order, fault)
            rl, rg, _ = rc.xent_ref(x, lab)
            worst = max(worst, rc.excess(loss, rl, 1e-5, 1e-5, rc.xent_loss_extra(x)))
            worst = max(worst, rc.xent_grad_excess(grad, rg, rc.f32(1.0 / M), F32, x))
            if fault is None:
                over = ((loss.double() - rl).abs() - (1e-5 + 1e-5 * rl.abs())).clamp(min=0)
                raw = max(raw, float((over / rc.xent_loss_extra(x, c=1.0)).max()))
    return worst, raw


def test_rowwise_emulators_pass_and_measure_the_allowance_constants():
    """Fault-free, every emulator passes every case inside the allowance, in both summation orders; and the constants in rowwise_cases are
    what this measurement gives: the next power of two above the worst ratio, times 4."""
    fwd, bwd, xe = [], [], []
    for order in ("lane", "seq"):
        w, r = _ln_emu_ratios(order)
        assert w <= 1.0, ("LayerNorm forward emulator", order, w)
        fwd.append(r)
        w, r = _ln_bwd_emu_ratios(order)
        assert w <= 1.0, ("LayerNorm backward emulator", order, w)
        bwd.append(r)
        w, r = _xent_emu_ratios(order)
        assert w <= 1.0, ("cross-entropy emulator", order, w)
        xe.append(r)
    print("worst raw ratios (lane, seq): forward %s backward %s xent %s" % (fwd, bwd, xe))
    assert rc.LN_C == 4 * _pow2_at_least(max(fwd)), fwd
    assert rc.LN_BWD_C == 4 * _pow2_at_least(max(bwd)), bwd
    assert rc.XENT_C == 4 * _pow2_at_least(max(xe)), xe


def test_rowwise_emulators_of_the_token_maps_and_the_chunk_walk_pass():
    g, b = rc.ln_params(0)
    B, T, N = 2, 4, 9
    S = 1 + N * T
    for regime in rc.LN_REGIMES:
        eps = rc.LN_EPS[regime]
        x = rc.ln_rows(B * S, regime, seed=5).view(B, S, 768)
        d = rc.delta_rows(B * T * (N + 1), torch.bfloat16, seed=6)
        x2 = rc.pre_mlp_add(x, d.float(), B, T, N)
        r2 = rc.pre_mlp_add(x.double(), d.double(), B, T, N)
        assert rc.excess(x2, r2, 2e-5, 2e-5) <= 1.0
        y = rc.emu_ln(x2.view(-1, 768), g, b, eps)[0]
        assert rc.excess(y, rc.ln_ref(r2.view(-1, 768), g, b, eps)[0], *FWD32, rc.ln_fwd_extra(r2.view(-1, 768), g, eps)) <= 1.0, regime
    rows = 32769
    x = rc.ln_rows(rows, "mixed", seed=7)
    y = rc.emu_ln_grid(x, g, b, 1e-12, rc.ln_fwd_waves(rows))
    assert rc.excess(y, rc.ln_ref(x, g, b, 1e-12)[0], *FWD32, rc.ln_fwd_extra(x, g, 1e-12)) <= 1.0
    for n in rc.ADAMW_SMALL + rc.ADAMW_BIG:
        assert rc.adamw_coverage(n).all(), n
    for n, kw in ADAMW_EMU_CASES:
        assert _adamw_emu_excess(n, kw, None) <= 1.0, (n, kw)


ADAMW_BASE = dict(lr=1e-2, b1=0.9, b2=0.98, eps=1e-6, wd=0.01, step_size=1e-2)
ADAMW_EMU_CASES = [(n, {}) for n in rc.ADAMW_SMALL + (4 * 1024 * 3 + 7,)] + [(1025, dict(lr=0.1, wd=0.1, step_size=0.1)), (1031, dict(wd=0.0)),
                                                                              (1031, dict(max_norm=2.0)), (1031, dict(grad_scale=1.0 / 128))]


def _adamw_emu_excess(n, kw, fault):
    a = dict(ADAMW_BASE, **kw)
    ins = rc.adamw_inputs(n, seed=1)
    extra = dict(gnorm_sq=(ins[1].double() ** 2).sum().float(), max_norm=a.pop("max_norm")) if "max_norm" in a else {}
    extra.update(grad_scale=a.pop("grad_scale", 1.0))
    args = (a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["step_size"])
    got = rc.emu_adamw(*ins, *args, fault=fault, **extra)
    ref = rc.adamw_ref(*ins, *args, **extra)
    return rc.adamw_excess(got, ref, ins)


LN_FAULTS = ("var_e2", "no_eps", "skip_last_lane")
XENT_FAULTS = ("no_max", "max_pairs", "label_off")
ADAMW_FAULTS = ("drop_tail", "skip_second", "wd_first")


def test_rowwise_emulators_catch_planted_faults():
    """Each planted fault fails at least one case (worst err / allowed > 1); the names say what is planted (rowwise_cases emu_* docstrings)."""
    caught = {}
    for f in LN_FAULTS:
        caught[f] = _ln_emu_ratios("lane", f)[0]
    g, b = rc.ln_params(0)
    # the CLS frame mean divided by N instead of T (PRE_MLP add, T = 4, N = 9)
    B, T, N = 2, 4, 9
    S = 1 + N * T
    x = rc.ln_rows(B * S, "gauss", seed=5).view(B, S, 768)
    d = rc.delta_rows(B * T * (N + 1), torch.bfloat16, seed=6)
    caught["cls_div_n"] = rc.excess(rc.pre_mlp_add(x, d.float(), B, T, N, div=N), rc.pre_mlp_add(x.double(), d.double(), B, T, N), 2e-5, 2e-5)
    # a wave that stops after its first trip: only the shape above 32768 rows can see it
    rows = 32769
    x = rc.ln_rows(rows, "mixed", seed=7)
    ref = rc.ln_ref(x, g, b, 1e-12)[0]
    extra = rc.ln_fwd_extra(x, g, 1e-12)
    caught["one_trip"] = rc.excess(rc.emu_ln_grid(x, g, b, 1e-12, rc.ln_fwd_waves(rows), "one_trip"), ref, *FWD32, extra)
    small = rc.ln_rows(74, "mixed", seed=7)
    assert rc.excess(rc.emu_ln_grid(small, g, b, 1e-12, rc.ln_fwd_waves(74), "one_trip"), rc.ln_ref(small, g, b, 1e-12)[0], *FWD32,
                     rc.ln_fwd_extra(small, g, 1e-12)) <= 1.0, "74 rows (the old test's shape) cannot see a wave that stops early"
    for f in XENT_FAULTS:
        caught[f] = _xent_emu_ratios("lane", f)[0]
    for f in ADAMW_FAULTS:
        caught[f] = max(_adamw_emu_excess(n, kw, f) for n, kw in ADAMW_EMU_CASES)
    print("planted faults, worst err / allowed: " + ", ".join("%s %.3g" % kv for kv in caught.items()))
    for f, w in caught.items():
        assert w > 1.0, "planted fault %s passes every case (worst err / allowed %.3g)" % (f, w)
    assert len(caught) == 11
