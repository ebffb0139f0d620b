"""GPU: the row-wise kernels with a delicate reduction of their own -- the LayerNorm family (alpro_layernorm_fwd, alpro_add_layernorm_fwd,
alpro_add_layernorm_pre_mlp2, alpro_vit_final_pool, alpro_bert_embed_fwd, alpro_cls_mean_residual, alpro_layernorm_bwd,
alpro_layernorm_bwd_emit), the loss (alpro_softmax_xent) and the step epilogue (alpro_sumsq, alpro_adamw_step, alpro_adamw_step_lp,
alpro_loss_scale_update) -- against torch fp64 on the CPU, on the stress regimes, shapes and edges of tests/rowwise_cases.py.  The allowances
are the project's tolerances plus the input-dependent conditioning terms derived there on the CPU (tests/test_rowwise_cases_cpu.py)."""
import pytest
import torch

from tests import rowwise_cases as rc
from tests.test_hip_bwd_ops import _determinism, _keep_mask
from tests.test_hip_ops import DTYPES, OUT_TOL, _hip

pytestmark = pytest.mark.gpu

D = 768
F32, F64 = torch.float32, torch.float64
TOL32 = (1e-5, 1e-5)       # fp32 LayerNorm outputs and statistics
TOLX = (2e-5, 2e-5)        # x' of the fused residual add
BWD_DX, BWD_DG = (1e-4, 2e-4), (1e-4, 2e-3)
SHAPES = [(2, 4, 9), (1, 1, 1), (3, 3, 5), (2, 5, 7)]
BIG = (21, 8, 196)         # 21 * 1569 = 32949 token rows: past the first trip of the forward kernels' 32768 waves


def dev(*ts):
    r = tuple(t.cuda() if t is not None else None for t in ts)
    return r if len(r) > 1 else r[0]


def all_dtypes_delta(rows, seed):
    """Gaussian on the 2^-3 grid: exact in fp32, bf16 and fp16 alike, so one fp64 reference serves the three dtypes."""
    return rc.on_grid(torch.randn(rows, D, generator=rc._gen(6000 + seed)), 2.0 ** -3)


def token_index(mode, B, T, N):
    """Token row (of the flat (B*S, D) stream) behind every row of a mapped LayerNorm: 'identity', 'skip' (x[:, 1:]), 'frame'."""
    S = 1 + N * T
    idx = torch.arange(B * S).view(B, S, 1)
    if mode == "identity":
        return idx.flatten()
    if mode == "skip":
        return idx[:, 1:].flatten()
    return rc.frame_gather(idx, B, T, N).flatten()


def map_kw(hip, mode, T, N):
    return {"identity": {}, "skip": dict(map_mode=hip.MAP_SKIP_CLS, map_p0=N * T), "frame": dict(map_mode=hip.MAP_FRAME_TOKENS, map_p0=T, map_p1=N)}[mode]


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def check_layernorm_maps(hip, x, eps, dts, B, T, N, seed=0):
    """alpro_layernorm_fwd on token rows x (B*S, 768): identity with the fp32 copy and the statistics, and the two gathers, every row."""
    g, b = rc.ln_params(seed)
    ry, rm, rr = rc.ln_ref(x, g, b, eps)
    ex = rc.ln_fwd_extra(x, g, eps)
    em, er = rc.ln_stats_extra(x, eps)
    xc, gc, bc = dev(x, g, b)
    for dt in dts:
        y, y32, mean, rstd = hip.layernorm(xc, gc, bc, eps, dt, out32=True, stats=True)
        rc.check(y, ry, *OUT_TOL[dt], ex, "ln identity y %s" % dt)
        if dt == dts[0]:
            rc.check(y32, ry, *TOL32, ex, "ln identity y32")
            rc.check(mean, rm, *TOL32, em, "ln mean")
            rc.check(rstd, rr, *TOL32, er, "ln rstd")
        else:
            assert torch.equal(y32, first32), "the fp32 copy depends on the 16-bit output dtype"
        first32 = y32
        for mode in (("skip", "frame") if dt == dts[0] or len(x) < 30000 else ()):     # big shape: the gathers once, in the first dtype
            idx = token_index(mode, B, T, N)
            y = hip.layernorm(xc, gc, bc, eps, dt, rows=idx.numel(), **map_kw(hip, mode, T, N))
            rc.check(y, ry[idx], *OUT_TOL[dt], ex[idx], "ln %s %s" % (mode, dt))


@pytest.mark.parametrize("regime", rc.LN_REGIMES)
@pytest.mark.parametrize("dt", DTYPES)
def test_layernorm_fwd_regimes_and_maps(dt, regime):
    hip = _hip()
    eps = rc.LN_EPS[regime]
    for k, (B, T, N) in enumerate(SHAPES):
        check_layernorm_maps(hip, rc.ln_rows(B * (1 + N * T), regime, seed=10 + k), eps, [dt], B, T, N)
    g, b = rc.ln_params(1)
    for rows in (1, 3, 5):
        x = rc.ln_rows(rows, regime, seed=20 + rows)
        y, y32 = hip.layernorm(*dev(x, g, b), eps, dt, out32=True)
        ref = rc.ln_ref(x, g, b, eps)[0]
        rc.check(y, ref, *OUT_TOL[dt], rc.ln_fwd_extra(x, g, eps), "ln %d rows" % rows)
        rc.check(y32, ref, *TOL32, rc.ln_fwd_extra(x, g, eps), "ln %d rows y32" % rows)


@pytest.mark.parametrize("regime", rc.LN_REGIMES)
def test_layernorm_fwd_past_the_first_grid_trip(regime):
    """32949 token rows (and 32769 identity rows): rows 32768.. are the second trip of the grid-stride loop; every row against fp64."""
    hip = _hip()
    B, T, N = BIG
    check_layernorm_maps(hip, rc.ln_rows(B * (1 + N * T), regime, seed=30), rc.LN_EPS[regime], DTYPES, B, T, N)
    if regime == "mixed":
        g, b = rc.ln_params(2)
        x = rc.ln_rows(32769, regime, seed=31)
        y = hip.layernorm(*dev(x, g, b), 1e-12, F32)
        rc.check(y, rc.ln_ref(x, g, b, 1e-12)[0], *TOL32, rc.ln_fwd_extra(x, g, 1e-12), "ln 32769 rows")


def add_ln_case(hip, mode, x, d, bias, B, T, N):
    """-> (hip mode, fp64 x' (B, S, D), index of the token row behind every y row) for add_layernorm mode 'identity' / 'pre_spatial' /
    'pre_mlp' / 'pre_temporal'; x (B, S, D) fp64, d the delta rows fp64, bias fp64 or None."""
    S = 1 + N * T
    bz = bias if bias is not None else torch.zeros(D, dtype=F64)
    if mode == "identity":
        return hip.ADD_IDENTITY, x + d.view(B, S, D) + bz, token_index("identity", B, T, N)
    if mode == "pre_spatial":
        xo = x.clone()
        xo[:, 1:] += d.view(B, N * T, D) + bz
        return hip.ADD_PRE_SPATIAL, xo, token_index("frame", B, T, N)
    if mode == "pre_mlp":      # the bias goes with the delta ROWS (the patches); the CLS row gets the frame mean of the deltas only
        xo = rc.pre_mlp_add(x, d, B, T, N)
        xo[:, 1:] += bz
        return hip.ADD_PRE_MLP, xo, token_index("identity", B, T, N)
    return hip.ADD_PRE_TEMPORAL, x + d.view(B, S, D) + bz, token_index("skip", B, T, N)


ADD_MODES = ("identity", "pre_spatial", "pre_mlp", "pre_temporal")
ADD_ROWS = {"identity": lambda B, T, N: B * (1 + N * T), "pre_spatial": lambda B, T, N: B * N * T, "pre_mlp": lambda B, T, N: B * T * (N + 1),
            "pre_temporal": lambda B, T, N: B * (1 + N * T)}


def check_add_layernorm(hip, x, regime, dts, B, T, N, deltas=None, variants=True):
    S = 1 + N * T
    eps = rc.LN_EPS[regime]
    g, b = rc.ln_params(3)
    bias = rc.on_grid(0.2 * torch.randn(D, generator=rc._gen(77)), 2.0 ** -10)
    xc, gc, bc, biasc = dev(x, g, b, bias)
    for mi, mode in enumerate(ADD_MODES):
        for with_bias in ((False, True) if deltas is None else (True,)):
            for dt in dts:
                if deltas is None or dt == dts[0]:     # shared deltas are exact in every dtype: one reference serves them all
                    d = deltas[mode] if deltas is not None else rc.delta_rows(ADD_ROWS[mode](B, T, N), dt, seed=40 + mi)
                    hmode, rx, idx = add_ln_case(hip, mode, x.double().view(B, S, D), d.double(), bias.double() if with_bias else None, B, T, N)
                    rx = rx.view(-1, D)
                    ry = rc.ln_ref(rx, g, b, eps)[0][idx]
                    ex = rc.ln_fwd_extra(rx, g, eps)[idx]
                kw = dict(mode=hmode, delta_bias=biasc if with_bias else None, T=T, N=N)
                dc = d.to(dt).cuda()
                y, y32, xo = hip.add_layernorm(xc, dc, gc, bc, eps, out32=True, **kw)
                what = "add_ln %s bias=%s %s" % (mode, with_bias, dt)
                rc.check(xo.view(-1, D), rx, *TOLX, 0.0, what + " x'")
                rc.check(y, ry, *OUT_TOL[dt], ex, what + " y")
                rc.check(y32, ry, *TOL32, ex, what + " y32")
                if variants:
                    xi = xc.clone()
                    y2, xo2 = hip.add_layernorm(xi, dc, gc, bc, eps, x_out=xi, **kw)
                    assert xo2 is xi and torch.equal(xi.view(-1, D), xo.view(-1, D)) and torch.equal(y2, y), what + " in place"
                    y3, none = hip.add_layernorm(xc, dc, gc, bc, eps, want_x=False, **kw)
                    assert none is None and torch.equal(y3, y), what + " want_x=False"


@pytest.mark.parametrize("regime", rc.LN_REGIMES)
@pytest.mark.parametrize("dt", DTYPES)
def test_add_layernorm_regimes_and_modes(dt, regime):
    hip = _hip()
    for k, (B, T, N) in enumerate(SHAPES):
        check_add_layernorm(hip, rc.ln_rows(B * (1 + N * T), regime, seed=50 + k), regime, [dt], B, T, N)


def test_add_layernorm_past_the_first_grid_trip():
    """The four modes at 32949 token rows, `mixed` rows (neighbours from different regimes), one delta exact in all three dtypes."""
    hip = _hip()
    B, T, N = BIG
    deltas = {m: all_dtypes_delta(ADD_ROWS[m](B, T, N), i) for i, m in enumerate(ADD_MODES)}
    check_add_layernorm(hip, rc.ln_rows(B * (1 + N * T), "mixed", seed=60), "mixed", DTYPES, B, T, N, deltas=deltas, variants=False)


@pytest.mark.parametrize("regime", rc.LN_REGIMES)
@pytest.mark.parametrize("dt", DTYPES)
def test_add_layernorm_pre_mlp2(dt, regime):
    """alpro_add_layernorm_pre_mlp2 against the reference algebra in fp64 (x + delta_t + bias on the patch rows, then the PRE_MLP scatter
    and the CLS frame mean), and bit for bit the pair add_layernorm(PRE_SPATIAL) -> add_layernorm(PRE_MLP) it stands for."""
    hip = _hip()
    eps = rc.LN_EPS[regime]
    g, b = rc.ln_params(4)
    bias = rc.on_grid(0.2 * torch.randn(D, generator=rc._gen(78)), 2.0 ** -10)
    for k, (B, T, N) in enumerate(SHAPES + ([BIG] if regime == "mixed" else [])):
        S = 1 + N * T
        x = rc.ln_rows(B * S, regime, seed=70 + k)
        dtm, dsp = rc.delta_rows(B * N * T, dt, seed=71 + k), rc.delta_rows(B * T * (N + 1), dt, seed=72 + k)
        for with_bias in ((True, False) if (B, T, N) != BIG else (True,)):
            rx = x.double().view(B, S, D).clone()
            rx[:, 1:] += dtm.double().view(B, N * T, D) + (bias.double() if with_bias else 0.0)
            rx = rc.pre_mlp_add(rx, dsp.double(), B, T, N).view(-1, D)
            xc, dtc, dsc, gc, bc, biasc = dev(x, dtm, dsp, g, b, bias if with_bias else None)
            xo = torch.empty_like(xc)
            y = hip.add_layernorm_pre_mlp2(xc, dtc, biasc, dsc, gc, bc, eps, T, N, x_out=xo)
            what = "pre_mlp2 %s bias=%s %s" % ((B, T, N), with_bias, dt)
            rc.check(xo, rx, *TOLX, 0.0, what + " x'")
            rc.check(y, rc.ln_ref(rx, g, b, eps)[0], *OUT_TOL[dt], rc.ln_fwd_extra(rx, g, eps), what + " y")
            _, x1 = hip.add_layernorm(xc, dtc, gc, bc, eps, mode=hip.ADD_PRE_SPATIAL, delta_bias=biasc, T=T, N=N)
            y2, x2 = hip.add_layernorm(x1, dsc, gc, bc, eps, mode=hip.ADD_PRE_MLP, T=T, N=N)
            assert torch.equal(x2.view(-1, D), xo) and torch.equal(y2, y), what + ": not the PRE_SPATIAL + PRE_MLP pair bit for bit"
            xi = xc.clone()
            y3 = hip.add_layernorm_pre_mlp2(xi, dtc, biasc, dsc, gc, bc, eps, T, N)
            assert torch.equal(xi, xo) and torch.equal(y3, y), what + " in place"


@pytest.mark.parametrize("regime", rc.LN_REGIMES)
@pytest.mark.parametrize("dt", DTYPES)
def test_vit_final_pool_and_cls_mean_residual(dt, regime):
    hip = _hip()
    eps = rc.LN_EPS[regime]
    g, b = rc.ln_params(5)
    B, N = 3, 5
    for T in (1, 3, 8):
        S = 1 + N * T
        x = rc.ln_rows(B * S, regime, seed=80 + T)
        ln = rc.ln_ref(x, g, b, eps)[0].view(B, S, D)
        ex = rc.ln_fwd_extra(x, g, eps).view(B, S, 1)
        ref = torch.cat([ln[:, :1], ln[:, 1:].reshape(B, N, T, D).mean(2)], 1)
        exo = torch.cat([ex[:, :1], ex[:, 1:].reshape(B, N, T, 1).amax(2)], 1)
        o32, ot = hip.vit_final_pool(*dev(x.view(B, S, D), g, b), eps, B, T, N, dt)
        rc.check(o32, ref, *TOL32, exo, "vit_final_pool fp32 T=%d" % T)
        rc.check(ot, ref, *OUT_TOL[dt], exo, "vit_final_pool %s T=%d" % (dt, T))
        if dt == F32:
            # alpro_cls_mean_residual, in place: T + 1 fp32 additions and one division, each rounding a partial sum no larger than
            # |x| + sum_t |side|: (T + 2) * 2^-24 of that is what the format allows
            side = rc.ln_rows(B * T, regime, seed=90 + T)
            xs = x.view(B, S, D)
            bound = (T + 2) * rc.U24 * (xs[:, 0].double().abs() + side.double().view(B, T, D).abs().sum(1))
            xi = xs.cuda().clone()
            out = hip.cls_mean_residual(xi, side.cuda(), xi, B, T)
            assert out is xi
            rc.check(xi[:, 0], xs[:, 0].double() + side.double().view(B, T, D).sum(1) / T, 1e-6, 1e-6, bound, "cls_mean_residual T=%d" % T)
            assert torch.equal(xi[:, 1:].cpu(), xs[:, 1:]), "cls_mean_residual touched a patch row"


@pytest.mark.parametrize("regime", rc.LN_REGIMES)
@pytest.mark.parametrize("dt", DTYPES)
def test_bert_embed_regimes_stats_and_dropout(dt, regime):
    """alpro_bert_embed_fwd: word rows from the regime, ids that hit row 0 and the last row of the table, row counts that are not multiples
    of 4, the statistics the backward reads, and the dropout form on an `outlier` table."""
    hip = _hip()
    eps = rc.LN_EPS[regime]
    g, b = rc.ln_params(6)
    Vw = 301
    word = rc.ln_rows(Vw, regime, seed=100)
    pos = rc.on_grid(0.5 * torch.randn(200, D, generator=rc._gen(101)), 2.0 ** -10)
    typ = rc.on_grid(0.5 * torch.randn(2, D, generator=rc._gen(102)), 2.0 ** -10)
    for L in (1, 30, 197):
        ids = torch.randint(0, Vw, (3, L), generator=rc._gen(103 + L))
        ids[0, 0], ids[2, L - 1] = 0, Vw - 1
        e = (word[ids].double() + typ[0].double() + pos[:L].double()).view(-1, D)
        ry, rm, rr = rc.ln_ref(e, g, b, eps)
        ex = rc.ln_fwd_extra(e, g, eps)
        em, er = rc.ln_stats_extra(e, eps)
        y32, yt, mean, rstd = hip.bert_embed(*dev(ids, word, pos, typ, g, b), eps, dt, stats=True)
        rc.check(y32, ry, *TOL32, ex, "bert_embed y32 L=%d" % L)
        rc.check(yt, ry, *OUT_TOL[dt], ex, "bert_embed %s L=%d" % (dt, L))
        rc.check(mean, rm, *TOL32, em, "bert_embed mean L=%d" % L)
        rc.check(rstd, rr, *TOL32, er, "bert_embed rstd L=%d" % L)
    if regime == "outlier":
        p, seed, L = 0.1, 4242, 30
        keep = _keep_mask(seed, 3 * L * D, p).view(3 * L, D).double()
        ids = torch.randint(0, Vw, (3, L), generator=rc._gen(110))
        e = (word[ids].double() + typ[0].double() + pos[:L].double()).view(-1, D)
        ref = rc.ln_ref(e, g, b, eps)[0] * keep / (1 - rc.f32(p))
        ex = rc.ln_fwd_extra(e, g, eps) / (1 - p)
        y32, yt = hip.bert_embed(*dev(ids, word, pos, typ, g, b), eps, dt, drop_p=p, drop_seed=seed)
        rc.check(y32, ref, *TOL32, ex, "bert_embed dropout y32")
        rc.check(yt, ref, *OUT_TOL[dt], ex, "bert_embed dropout %s" % dt)
        assert torch.equal(y32.cpu() == 0, keep == 0)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def ln_bwd_reference(x, dy, dy2, dres, g, eps, idx, accumulate, chunk=8192):
    """fp64, in row chunks: -> dx (tokens, D), dgamma, dbeta and their conditioning allowances (dx_extra (tokens, 1), dgamma_extra (D,))."""
    tokens = x.shape[0]
    scat = torch.zeros(tokens, D, dtype=F64)
    exs = torch.zeros(tokens, 1, dtype=F64)
    dgam, dbet, exg = torch.zeros(D, dtype=F64), torch.zeros(D, dtype=F64), torch.zeros(D, dtype=F64)
    for lo in range(0, idx.numel(), chunk):
        sl = slice(lo, lo + chunk)
        d = dy[sl].double() + (dy2[sl].double() if dy2 is not None else 0.0)
        xr = x[idx[sl]]
        dxr, ag = rc.ln_bwd_ref(xr, d, g, eps)
        scat.index_add_(0, idx[sl], dxr)
        exs.index_add_(0, idx[sl], rc.ln_dx_extra(xr, d, g, eps))
        dgam += ag.sum(0)
        dbet += d.sum(0)
        exg += rc.ln_dgamma_extra(xr, d, eps)
    touched = torch.zeros(tokens, dtype=torch.bool)
    touched[idx] = True
    base = dres.double() if accumulate else torch.zeros(tokens, D, dtype=F64)
    return torch.where(touched[:, None], base + scat, dres.double()), dgam, dbet, exs, exg


def run_ln_bwd(hip, x, dy, dy2, dres, g, eps, rows, accumulate, kw, emit=None):
    dx = dres.cuda().clone()
    dg, db = torch.full((D,), 0.5).cuda(), torch.full((D,), -0.25).cuda()     # accumulated onto, not overwritten
    r = hip.layernorm_bwd(dy.cuda(), x.cuda(), g.cuda(), eps, dx, dg, db, rows=rows, dy2=dy2.cuda() if dy2 is not None else None,
                          accumulate=accumulate, emit=emit, **kw)
    return dx, dg, db, (r[1] if emit is not None else None)


def check_ln_bwd(got, ref, what):
    dx, dg, db, _ = got
    rdx, rdg, rdb, exs, exg = ref
    rc.check(dx, rdx, *BWD_DX, exs, what + " dx")
    rc.check(dg, 0.5 + rdg, *BWD_DG, exg, what + " dgamma")
    rc.check(db, -0.25 + rdb, *BWD_DG, 0.0, what + " dbeta")


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("regime", rc.LN_REGIMES)
@pytest.mark.parametrize("dt", DTYPES)
def test_layernorm_bwd_regimes_maps_and_grid_trips(dt, regime, det):
    """alpro_layernorm_bwd in its three maps on 348 token rows with the workgroup count capped at 1 and 3 (every wave walks 30 to 90 rows)
    and under the default plan, with a second gradient stream, accumulating and not: dx, dgamma, dbeta against fp64."""
    hip = _hip()
    eps = rc.LN_EPS[regime]
    g, _ = rc.ln_params(7)
    B, T, N = 6, 3, 19
    S = 1 + N * T
    x = rc.ln_rows(B * S, regime, seed=120)
    dres = rc.on_grid(torch.randn(B * S, D, generator=rc._gen(121)), 2.0 ** -10)
    with _determinism(hip, det):
        for mi, mode in enumerate(("identity", "skip", "frame")):
            idx = token_index(mode, B, T, N)
            rows = idx.numel()
            dy = rc.delta_rows(rows, dt, seed=122 + mi)
            dy2 = rc.on_grid(torch.randn(rows, D, generator=rc._gen(125 + mi)), 2.0 ** -10)
            for accumulate, second in ((True, True), (True, False)) + (((False, True),) if mode != "frame" else ()):
                ref = ln_bwd_reference(x.double(), dy, dy2 if second else None, dres, g, eps, idx, accumulate)
                for grid in (1, 3, 0):
                    with hip.option("ln_grid", grid):
                        got = run_ln_bwd(hip, x, dy, dy2 if second else None, dres, g, eps, rows, accumulate, map_kw(hip, mode, T, N))
                    check_ln_bwd(got, ref, "ln bwd %s acc=%s dy2=%s ln_grid=%d" % (mode, accumulate, second, grid))


def test_layernorm_bwd_default_plan_above_65536_rows():
    """66192 frame-token rows (112 clips of 3 frames x 196 patches): the default plan's 2048 workgroups take a second trip, dgamma / dbeta
    are summed over 2048 partials and every clip's CLS row over its frame terms -- all against fp64, in both determinism modes and the
    three gradient dtypes (one gradient that is exact in all of them)."""
    hip = _hip()
    B, T, N = 112, 3, 196
    S = 1 + N * T
    eps = 1e-6
    g, _ = rc.ln_params(8)
    idx = token_index("frame", B, T, N)
    rows = idx.numel()
    assert rows == 66192 and rows > 65536
    x = rc.ln_rows(B * S, "mixed", seed=130)
    dres = rc.on_grid(torch.randn(B * S, D, generator=rc._gen(131)), 2.0 ** -10)
    dy = all_dtypes_delta(rows, 132)
    ref = ln_bwd_reference(x.double(), dy, None, dres, g, eps, idx, True)
    for det in (True, False):
        with _determinism(hip, det):
            for dt in DTYPES:
                got = run_ln_bwd(hip, x, dy.to(dt), None, dres, g, eps, rows, True, map_kw(hip, "frame", T, N))
                check_ln_bwd(got, ref, "ln bwd 66192 rows det=%s %s" % (det, dt))


@pytest.mark.parametrize("regime", ("gauss", "outlier", "mixed"))
@pytest.mark.parametrize("dt", DTYPES)
def test_layernorm_bwd_emit_against_fp64(dt, regime):
    """alpro_layernorm_bwd_emit: the operand rows of the three emit modes against fp64 directly (T = 3).  Under the ViT's eps = 1e-6, whose
    hand-overs these are: with 1e-12 a constant row has rstd = 1e6 and its gradient row leaves fp16's range, in the reference as well."""
    hip = _hip()
    eps = 1e-6
    g, _ = rc.ln_params(9)
    B, T, N = 4, 3, 7
    S = 1 + N * T
    x = rc.ln_rows(B * S, regime, seed=140)
    dres = rc.on_grid(torch.randn(B * S, D, generator=rc._gen(141)), 2.0 ** -10)
    gen = rc._gen(142)
    sc_bt = (torch.rand(B * T, generator=gen) > 0.3).float() / 0.75
    sc_bn = (torch.rand(B * N, generator=gen) > 0.3).float() / 0.75
    sc_b = (torch.rand(B, generator=gen) > 0.3).float() / 0.75

    def emitted(got, ref, scale_rows, src_rows, what):
        """got: emitted (rows, D) in dt; expected = dx_ref[src_rows] * scale_rows."""
        rdx, exs = ref[0], ref[3]
        rc.check(got, rdx[src_rows] * scale_rows[:, None].double(), OUT_TOL[dt][0] + BWD_DX[0], BWD_DX[1] * float(scale_rows.max()),
                 exs[src_rows] * scale_rows[:, None].double(), what)

    # identity-map backward -> frame-token operand rows, the CLS row to every frame at 1 / T
    idx = token_index("identity", B, T, N)
    dy = rc.delta_rows(B * S, dt, seed=143)
    ref = ln_bwd_reference(x.double(), dy, None, dres, g, eps, idx, True)
    got = run_ln_bwd(hip, x, dy, None, dres, g, eps, B * S, True, {}, emit=dict(mode=hip.EMIT_FRAME, rows=B * T * (N + 1), dtype=dt, T=T, N=N, scale=sc_bt.cuda()))
    check_ln_bwd(got, ref, "emit frame")
    fidx = token_index("frame", B, T, N)
    is_cls = (torch.arange(B * T * (N + 1)) % (N + 1)) == 0
    scale = sc_bt.repeat_interleave(N + 1) * torch.where(is_cls, torch.tensor(rc.f32(1.0 / T)), torch.tensor(1.0))
    emitted(got[3], ref, scale, fidx, "emit frame rows")
    # frame-map backward -> x[:, 1:] operand rows + the unscaled column sums
    dy = rc.delta_rows(B * T * (N + 1), dt, seed=144)
    ref = ln_bwd_reference(x.double(), dy, None, dres, g, eps, fidx, True)
    cs = torch.full((D,), 2.0).cuda()
    got = run_ln_bwd(hip, x, dy, None, dres, g, eps, fidx.numel(), True, map_kw(hip, "frame", T, N),
                     emit=dict(mode=hip.EMIT_SKIP_CLS, rows=B * N * T, dtype=dt, T=T, N=N, scale=sc_bn.cuda(), group=T, colsum_pre=cs))
    check_ln_bwd(got, ref, "emit skip_cls")
    sidx = token_index("skip", B, T, N)
    emitted(got[3], ref, sc_bn.repeat_interleave(T), sidx, "emit skip_cls rows")
    rc.check(cs, 2.0 + ref[0][sidx].sum(0), *BWD_DG, ref[3][sidx].sum(0), "emit skip_cls colsum_pre")
    # skip-map backward -> every token row, the CLS rows it never touched included
    dy = rc.delta_rows(B * N * T, dt, seed=145)
    ref = ln_bwd_reference(x.double(), dy, None, dres, g, eps, sidx, True)
    got = run_ln_bwd(hip, x, dy, None, dres, g, eps, sidx.numel(), True, map_kw(hip, "skip", T, N),
                     emit=dict(mode=hip.EMIT_ROWS, rows=B * S, dtype=dt, T=T, N=N, scale=sc_b.cuda(), group=S, extra_cls=B))
    check_ln_bwd(got, ref, "emit rows")
    emitted(got[3], ref, sc_b.repeat_interleave(S), torch.arange(B * S), "emit rows rows")


# ------------------------------------------------------------------------------------------------ cross-entropy
def run_xent(hip, x, labels, dt, scale, strided, ignore_index=-100):
    """-> loss_rows, dl (M, Vpad).  strided: the logits are the first V columns of a (M, Vpad) buffer whose other columns hold 1e30."""
    M, V = x.shape
    if strided:
        Vp = (V + 63) // 64 * 64 + (64 if V % 64 == 0 else 0)
        buf = torch.full((M, Vp), 1e30)
        buf[:, :V] = x
        xc = buf.cuda()[:, :V]
        assert xc.stride(0) == Vp
    else:
        xc = x.cuda()
    return hip.softmax_xent(xc, labels.cuda(), grad_dtype=dt, grad_scale=torch.tensor([scale], dtype=F32).cuda(), ignore_index=ignore_index)


@pytest.mark.parametrize("V", rc.XENT_V)
@pytest.mark.parametrize("dt", DTYPES)
def test_softmax_xent_regimes_widths_and_scales(dt, V):
    """alpro_softmax_xent over the regimes, M in (1, 83), the gradient in dt scaled by 1/n and by 2^16/n (the fp16 mode's pre-multiplied
    loss scale).  Odd V runs as a row-strided view, even V contiguous (and strided once)."""
    hip = _hip()
    for M in (1, 83):
        for regime in rc.XENT_REGIMES:
            x, labels = rc.xent_inputs(M, V, regime, seed=3)
            rl, rg, n = rc.xent_ref(x, labels)
            assert n == M
            layouts = (True,) if V % 2 else ((False, True) if regime == "late_max" else (False,))
            for strided in layouts:
                for mult in (1.0, 65536.0):
                    scale = rc.f32(mult / n)
                    loss, dl = run_xent(hip, x, labels, dt, scale, strided)
                    what = "xent M=%d V=%d %s strided=%s scale=%g %s" % (M, V, regime, strided, scale, dt)
                    rc.check(loss, rl, 1e-5, 1e-5, rc.xent_loss_extra(x), what + " loss_rows")
                    assert dl.shape == (M, (V + 63) // 64 * 64) and dl.dtype == dt
                    assert float(dl[:, V:].float().abs().sum()) == 0, what + ": pad columns not zero"
                    r = rc.xent_grad_excess(dl[:, :V], rg, scale, dt, x)
                    assert r <= 1.0, "%s gradient: worst error is %.3g x the allowance" % (what, r)


@pytest.mark.parametrize("dt", DTYPES)
def test_softmax_xent_ignored_rows_and_refused_layouts(dt):
    hip = _hip()
    for V, strided in ((65, True), (3129, True), (1500, False)):
        M = 83
        x, labels = rc.xent_inputs(M, V, "gauss", seed=4)
        cases = [("all ignored", torch.full((M,), -100), -100), ("none ignored", labels, -100)]
        some = labels.clone()
        some[::3] = -100
        cases.append(("every third ignored", some, -100))
        zero = labels.clone()
        zero[5::4] = 0           # ignore_index = 0: label 0 (a real column elsewhere) marks the ignored rows
        cases.append(("ignore_index 0", zero, 0))
        for name, lab, ign in cases:
            rl, rg, n = rc.xent_ref(x, lab, ignore_index=ign)
            scale = rc.f32(1.0 / max(n, 1))
            loss, dl = run_xent(hip, x, lab, dt, scale, strided, ignore_index=ign)
            what = "xent V=%d %s %s" % (V, name, dt)
            rc.check(loss, rl, 1e-5, 1e-5, rc.xent_loss_extra(x), what + " loss_rows")
            ignored = (lab == ign)
            assert (loss.cpu()[ignored] == 0).all(), what + ": loss_rows of an ignored row"
            assert float(dl[:, V:].float().abs().sum()) == 0 and float(dl.cpu()[ignored].float().abs().sum()) == 0, what + ": pad columns / ignored rows not zero"
            assert rc.xent_grad_excess(dl[:, :V], rg, scale, dt, x) <= 1.0, what + " gradient"
        assert name == "ignore_index 0" and int(ignored.sum()) > 15 and n < M
    one = torch.tensor([1.0]).cuda()
    for M in (1, 83):        # a contiguous odd-V tensor has rows at odd offsets: refused, not read through misaligned pairs
        with pytest.raises(RuntimeError, match="8-byte aligned"):
            hip.softmax_xent(torch.zeros(M, 65).cuda(), torch.zeros(M, dtype=torch.int64).cuda(), grad_dtype=dt, grad_scale=one)


# ------------------------------------------------------------------------------------------------ optimizer epilogue
ADAMW_ARGS = dict(lr=1e-2, b1=0.9, b2=0.98, eps=1e-6, wd=0.01, step_size=1e-2)
SENTINEL = 12345.0


def run_adamw(hip, ins, n, a, lp_dt=None, **kw):
    """The kernel on the first n elements of buffers 64 elements longer, the rest holding a sentinel.  -> p, m, v (n,), lp or None."""
    bufs = []
    for t in ins:
        buf = torch.full((n + 64,), SENTINEL).cuda()
        buf[:n] = t.cuda()
        bufs.append(buf)
    lp = torch.full((n + 64,), SENTINEL, dtype=lp_dt).cuda() if lp_dt is not None else None
    p, g, m, v = (buf[:n] for buf in bufs)
    hip.adamw_step(p, g, m, v, a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["step_size"], lp=lp[:n] if lp is not None else None, **kw)
    for buf in bufs + ([lp] if lp is not None else []):
        assert (buf[n:] == SENTINEL).all(), "adamw wrote past n=%d" % n
    assert torch.equal(g.cpu(), ins[1]), "adamw changed the gradient without zero_grad"
    return p, m, v, (lp[:n] if lp is not None else None)


@pytest.mark.parametrize("n", rc.ADAMW_SMALL + rc.ADAMW_BIG)
def test_adamw_step_sizes_and_mirror(n):
    """alpro_adamw_step / alpro_adamw_step_lp at the edges of the chunk walk: below one float4, around one workgroup, and around one, two
    and three capped trips of S = rc.ADAMW_S = 4 194 304 elements (optim.hip grid_for caps the grid at 4096 workgroups)."""
    hip = _hip()
    ins = rc.adamw_inputs(n, seed=2)
    norm = (ins[1].double() ** 2).sum().float().reshape(1)
    a = ADAMW_ARGS
    ref = rc.adamw_ref(*ins, a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["step_size"], gnorm_sq=norm, max_norm=2.0)
    lp_dt = torch.float16 if n % 2 else torch.bfloat16
    plain = run_adamw(hip, ins, n, a, gnorm_sq=norm.cuda(), max_norm=2.0)
    r = rc.adamw_excess(plain[:3], ref, ins)
    assert r <= 1.0, "adamw n=%d: worst error is %.3g x the allowance" % (n, r)
    mirrored = run_adamw(hip, ins, n, a, lp_dt=lp_dt, gnorm_sq=norm.cuda(), max_norm=2.0)
    for x, y, what in zip(plain[:3], mirrored[:3], "pmv"):
        assert torch.equal(x, y), "adamw n=%d: %s differs with the 16-bit mirror" % (n, what)
    assert torch.equal(mirrored[3], hip.cast(mirrored[0].clone(), lp_dt)), "adamw n=%d: mirror != cast of the updated parameters" % n


ADAMW_SWITCHES = [
    dict(wd=0.0), dict(correct_bias=False, dyn=(1.0, 0.0, 9.0, 0.0)), dict(max_norm=0.0), dict(gnorm=False), dict(grad_scale=1.0 / 128),
    dict(lr=0.1, wd=0.1, step_size=0.1),
] + [dict(dyn=(1024.0, 5.0, steps, 1.0), grads_scaled=gs) for steps in (0.0, 9.0, 9999.0) for gs in (True, False)]


@pytest.mark.parametrize("sw", ADAMW_SWITCHES, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()).replace(" ", ""))
def test_adamw_step_switches(sw):
    """One switch at a time at a ragged size, against the reference update (tests/test_hip_bwd_ops.py::test_flat_adamw_matches_reference_update)."""
    hip = _hip()
    n = 256 * 4 * 3 + 4 * 5 + 3
    sw = dict(sw)
    a = dict(ADAMW_ARGS, **{k: sw.pop(k) for k in list(sw) if k in ADAMW_ARGS})
    ins = rc.adamw_inputs(n, seed=3)
    dyn = sw.pop("dyn", None)
    if dyn is not None and sw.get("grads_scaled", True):
        ins = (ins[0], ins[1] * dyn[0], ins[2], ins[3])      # the gradients arrive multiplied by the loss scale
    norm = (ins[1].double() ** 2).sum().float().reshape(1) if sw.pop("gnorm", True) else None
    max_norm = sw.pop("max_norm", 2.0)
    kw = dict(gnorm_sq=norm, max_norm=max_norm, **sw)
    ref = rc.adamw_ref(*ins, a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["step_size"], dyn=dyn, **kw)
    dync = torch.tensor(dyn).cuda() if dyn is not None else None
    got = run_adamw(hip, ins, n, a, dyn_state=dync, **dict(kw, gnorm_sq=norm.cuda() if norm is not None else None))
    r = rc.adamw_excess(got[:3], ref, ins)
    assert r <= 1.0, "adamw switches: worst error is %.3g x the allowance" % r
    if dync is not None:
        assert dync.tolist() == list(dyn), "adamw_step changed the loss-scaler state"


@pytest.mark.parametrize("n", rc.ADAMW_SMALL + rc.ADAMW_BIG)
def test_sumsq_sizes(n):
    """alpro_sumsq accumulating onto a non-zero `out`, both determinism modes.  Values near 1 with 1000 planted at the first and last element,
    the middle and the start of the ragged tail: an element left out moves the sum by more than the tolerance."""
    hip = _hip()
    x = rc.on_grid(1 + 0.5 * torch.rand(n, generator=rc._gen(7000 + n % 9973)), 2.0 ** -10)
    x[[0, n - 1, n // 2, (n - 1) // 4 * 4]] = 1000.0
    ref = 3.5 + float((x.double() ** 2).sum())
    xc = x.cuda()
    for det in (True, False):
        with _determinism(hip, det):
            out = torch.tensor([3.5]).cuda()
            hip.sumsq(xc, out)
            assert abs(float(out) - ref) <= 1e-5 * ref, "sumsq n=%d det=%s: %r vs %r" % (n, det, float(out), ref)


def test_loss_scale_update_clamps_and_window():
    """alpro_loss_scale_update on its own state words {scale, tracker, applied, skipped}.  (tests/test_amp_gpu.py already pins, through FlatAdamW
    and the default clamps: halving on an inf / NaN norm, the tracker restart and one doubling after a window of 2; not repeated here.)"""
    hip = _hip()

    def step(state, norm, **kw):
        hip.loss_scale_update(state, torch.tensor([norm]).cuda(), **kw)
        return state.tolist()

    st = torch.tensor([2.0, 5.0, 7.0, 1.0]).cuda()
    assert step(st, float("inf"), min_scale=1.5) == [1.5, 0.0, 7.0, 2.0]              # halving stops at min_scale ...
    assert step(st, float("nan"), min_scale=1.5) == [1.5, 0.0, 7.0, 3.0]              # ... and stays there; NaN counts as overflow too
    st = torch.tensor([2.0 ** 23, 2.0, 3.0, 0.0]).cuda()
    assert step(st, 1.0, window=3, max_scale=1.5 * 2.0 ** 23) == [1.5 * 2.0 ** 23, 0.0, 4.0, 0.0]   # doubling stops at max_scale
    for _ in range(2):
        assert step(st, 1.0, window=3, max_scale=1.5 * 2.0 ** 23)[0] == 1.5 * 2.0 ** 23
    assert step(st, 1.0, window=3, max_scale=1.5 * 2.0 ** 23) == [1.5 * 2.0 ** 23, 0.0, 7.0, 0.0]
    st = torch.tensor([8.0, 0.0, 0.0, 0.0]).cuda()
    seen = [step(st, 4.0, window=3) for _ in range(4)]
    assert seen == [[8.0, 1.0, 1.0, 0.0], [8.0, 2.0, 2.0, 0.0], [16.0, 0.0, 3.0, 0.0], [16.0, 1.0, 4.0, 0.0]]   # growth exactly at `window` clean steps
    assert step(st, float("inf"), window=3) == [8.0, 0.0, 4.0, 1.0]
    assert step(st, float("inf"), window=3, backoff=0.25, min_scale=1.0) == [2.0, 0.0, 4.0, 2.0]
    assert step(st, 4.0, window=1, growth=4.0) == [8.0, 0.0, 5.0, 2.0]
