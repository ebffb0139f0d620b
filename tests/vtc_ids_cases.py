"""Id patterns, the fp64 reference, an fp32 emulator and derived allowances for the video-text contrastive loss with video ids
(alpro_vtc_loss_ids_fwd / _bwd: vtc_ids_loss_finish_kernel and vtc_ids_bwd_rows_kernel of alpro_amd/csrc/loss.hip beside the plain loss's
forward, d temp and column kernels, behind _VtcLossIds).  Shared by tests/test_hip_vtc_ids_gpu.py, tests/test_vtc_ids_model_gpu.py (GPU) and
tests/test_vtc_ids_cpu.py (CPU self-check); not collected itself, and nothing here touches a GPU.  The inputs (rows on the 2^-10 grid, exact dot
products), the regimes and every helper come from tests/vtc_cases.py (`vc`), which stays as it is.

Contract (include/alpro_hip.h), the same in both directions; pair i owns one id for its video and its caption:
  match(i, j) = (j == col0 + i) || (ids[i] >= 0 && gids[j] == ids[i])      64-bit compare; a negative id matches nothing but its own column;
                                                                            the own column matches whatever gids[col0 + i] says
  n_i = #{j : match(i, j)} >= 1,   row_i = lse_i - (sum_{match} sim_ij) / n_i,   loss = sum_{dir, i} row_i / (2B)
  ds_ij = (exp(sim_ij - lse_i) - match(i, j) / n_i) * dloss / (2B);   dv, dt, dgv, dgt, dtemp from ds as in the plain loss.

Reference.  Written from this contract in fp64 (reference below): the loss as stated, the gradients by autograd, tc the leaf of d temp as in vc.

Allowances.  Those of vc.allowances (its docstring derives them) with the one-hot replaced by the target w_i match(i, j), w_i = 1 / n_i, and
the positive logit by the mean m_i = w_i sum_{match} sim_ij.  What the ids add, first order in u = 2^-24, every quantity from fp64:
  mean   the finishing kernel's wave adds the matching logits of a row: lane l the columns l, l + 64, ... in ascending order, then six
         butterfly steps, so a logit passes at most D = ceil(G / 64) + 6 additions, and no more than n_i - 1 of them have two non-zero
         operands (adding 0 is exact).  Then w_i = fl(1 / n_i) rounds once (u; exact for a power of two, taken as u whenever n_i > 1) and
         fl(S w_i) once more:
                 A_mean_i = w_i sum_{match} A_sim_ij + u (min(n_i - 1, D) + 2 [n_i > 1]) w_i sum_{match} |sim_ij|
         With n_i = 1 this is A_sim of the positive, vc's term.  The row term lse_i - m_i rounds by u |term| as before, and every term is still
         >= 0 (lse >= max >= mean), so vc's A_loss holds with A_mean in the place of A_sim_pos.
  ds     p - w_i match rounds by u |p - w_i match| (inside vc's 4 u |ds|); the target itself carries the rounding of 1 / n_i:
                 A_ds = vc's A_ds + u [n_i > 1] w_i match(i, j) |scale|
  dq, dk, dtemp: vc's formulas on this ds and A_ds (the chains and the finishing sums are the same kernels or the same loops).
The allowance of an output is C * A, C = vc.MARGIN * RECORDED, where RECORDED is MEASURED -- the largest error / A of the fault-free emulator
(emu below) against the fp64 reference over every case of cases() -- rounded up by about a tenth, as in vc and for vc's reasons (device expf /
logf, wave-tree order, FMA contraction).  tests/test_vtc_ids_cpu.py re-measures them on every run.
"""
from collections import namedtuple

import torch

from tests import vtc_cases as vc
from tests.rowwise_cases import wave_sum

F32, F64, I64 = torch.float32, torch.float64, torch.int64
U, TINY, MARGIN = vc.U, vc.TINY, vc.MARGIN

# (B, G, E, col0)
SHAPES = (
    (1, 1, 256, 0),            # loss and gradients exactly 0
    (3, 3, 256, 0),            # smallest shape with a duplicate
    (5, 13, 12, 8),            # col0 + B = G, matches only in other ranks' columns
    (5, 13, 4, 3),             # smallest E, col0 no multiple of B
    (130, 260, 64, 130),       # matches at columns >= 256: the second trip of the strided loops and of the finishing sum
    (16, 8192, 32, 8176),      # the backward's largest G
)
REGIMES = ("gauss", "dup", "late_neg_last")
TEMPS = (0.07, 0.001)
PATTERNS = ("distinct", "dup_local", "dup_outside", "all_equal", "negatives", "high_bits", "own_disagrees")
FAULTS = ("no_div", "own_dropped", "ids32", "neg_match")
OUTPUTS, SAVED, FAMILY = vc.OUTPUTS, vc.SAVED, vc.FAMILY
BASE = 1 << 20             # the distinct ids are BASE + column

# Largest error / A of the fault-free emulator against fp64 over SHAPES x REGIMES x TEMPS x PATTERNS with dloss = 1.7 and, on gauss, with
# vc.SCALED_DLOSS (tests/test_vtc_ids_cpu.py::test_emulator_stays_within_a_quarter_of_every_constant re-measures and prints them), and the
# constants: MARGIN x the measured value rounded up by about a tenth.
# Worst cases: sim (130, 260, 64) dup 0.001; lse (5, 13, 12) dup 0.001; loss (5, 13, 4) gauss 0.07 dup_outside; ds (3, 3, 256) late_neg_last
# 0.07 all_equal; dq (16, 8192, 32) dup 0.07 all_equal; dk (130, 260, 64) late_neg_last 0.07 distinct; dtemp (16, 8192, 32) late_neg_last 0.07.
MEASURED = {"sim": 0.6016, "lse": 0.6244, "loss": 0.1410, "ds": 0.5511, "dq": 0.6430, "dk": 1.1631, "dtemp": 0.0435}
RECORDED = {"sim": 0.66, "lse": 0.7, "loss": 0.155, "ds": 0.61, "dq": 0.71, "dk": 1.28, "dtemp": 0.048}       # MEASURED rounded up by about a tenth
C = {k: MARGIN * m for k, m in RECORDED.items()}       # sim 2.64, lse 2.8, loss 0.62, ds 2.44, dq 2.84, dk 5.12, dtemp 0.192

IdCase = namedtuple("IdCase", vc.Case._fields + ("pattern", "ids", "gids"))


def id_pattern(pattern, B, G, col0):
    """-> (ids (B,), gids (G,)) int64.  Where the shape has no room for the pattern (one pair; no column outside the own block) what is left of
    it is built: the case then repeats `distinct` or a weaker pattern, and still has to hold."""
    gids = BASE + torch.arange(G, dtype=I64)
    own = col0 + torch.arange(B)
    outside = [j for j in (0, col0 - 1, col0 + B, G - 1) if 0 <= j < G and not col0 <= j < col0 + B]
    if pattern == "distinct":
        pass
    elif pattern == "dup_local":                 # rows 0 and 1 (and the last two rows) share a video
        if B >= 2:
            gids[col0 + 1] = gids[col0]
        if B >= 4:
            gids[col0 + B - 1] = gids[col0 + B - 2]
    elif pattern == "dup_outside":               # rows 0 and B - 1 have a caption of their video on another rank, none on their own
        for k, j in enumerate(outside):
            gids[j] = gids[col0 if k % 2 == 0 else col0 + B - 1]
    elif pattern == "all_equal":                 # n_i = G: every row of ds sums to 0
        gids[:] = 7
    elif pattern == "negatives":                 # rows 0, 2, 4, ... and every third column have no id: they must not match each other
        gids[0::3] = -1
        gids[own[0::2]] = -1
        keep = [int(j) for j in own if gids[j] >= 0]
        if keep and outside:                     # ... and a row with an id still finds its copy
            gids[outside[0]] = gids[keep[0]]
    elif pattern == "high_bits":                 # equal low 32 bits, different ids
        gids[col0] = 5
        if B >= 2:
            gids[col0 + 1] = 5 + (1 << 32)
        for k, j in enumerate(outside):
            gids[j] = 5 + (1 << (33 + 7 * k))
    elif pattern == "own_disagrees":             # the gathered id of row 0's own column is another one, and row 0's id sits in an outside column
        ids = gids[own].clone()
        gids[col0] = 3
        if outside:
            gids[outside[-1]] = ids[0]
        return ids, gids
    else:
        raise ValueError(pattern)
    return gids[own].clone(), gids


def build(shape, regime, temp, pattern):
    c = vc.build(shape, regime, temp)
    ids, gids = id_pattern(pattern, c.B, c.G, c.col0)
    return IdCase(*c._replace(name=c.name + "-" + pattern), pattern, ids, gids)


def cases(shapes=SHAPES, regimes=REGIMES, temps=TEMPS, patterns=PATTERNS):
    for s in shapes:
        for r in regimes:
            for t in temps:
                for p in patterns:
                    yield build(s, r, t, p)


def dlosses(c):
    return (1.7, vc.SCALED_DLOSS) if c.regime == "gauss" else (1.7,)


def match(ids, gids, col0):
    """The contract's match(i, j) -> bool (B, G)."""
    B = ids.shape[0]
    m = (gids[None, :] == ids[:, None]) & (ids[:, None] >= 0)
    m[torch.arange(B), col0 + torch.arange(B)] = True
    return m


# ------------------------------------------------------------------------------------------------ fp64 reference
def loss64(v, t, gv, gt, tc, col0, ids, gids):
    """The contract in the dtype of its arguments -> (loss, sim_v2t, sim_t2v, lse (2B))."""
    B = v.shape[0]
    m = match(ids, gids, col0).to(v.dtype)
    n = m.sum(1)
    sv, st = v @ gt.t() / tc, t @ gv.t() / tc
    lv, lt = torch.logsumexp(sv, 1), torch.logsumexp(st, 1)
    loss = ((lv - (sv * m).sum(1) / n).sum() + (lt - (st * m).sum(1) / n).sum()) / (2 * B)
    return loss, sv, st, torch.cat([lv, lt])


def reference(c, dloss=1.0):
    """fp64 -> dict over OUTPUTS (gradients of dloss * loss; dtemp with respect to the clamped temperature)."""
    v, t, gv, gt = (x.double().requires_grad_(True) for x in (c.v, c.t, c.gv, c.gt))
    tc = vc.clamped(c.temp).double().requires_grad_(True)
    loss, sv, st, lse = loss64(v, t, gv, gt, tc, c.col0, c.ids, c.gids)
    (loss * dloss).backward()
    return dict(sim_v2t=sv.detach(), sim_t2v=st.detach(), lse=lse.detach(), loss=loss.detach(), dv=v.grad, dt=t.grad, dgv=gv.grad, dgt=gt.grad,
                dtemp=tc.grad)


# ------------------------------------------------------------------------------------------------ allowances
def allowances(c, dloss=1.0, ds64=None):
    """fp64 -> dict over OUTPUTS + SAVED of A (the module docstring and vc's), before the constant.  ds64: a dict that receives the fp64 ds."""
    ds64 = {} if ds64 is None else ds64
    B, G, col0 = c.B, c.G, c.col0
    tc = float(vc.clamped(c.temp))
    T = (G + 255) // 256
    D = (G + 63) // 64 + 6
    scale = abs(dloss) / (2 * B)
    m = match(c.ids, c.gids, col0).double()
    n = m.sum(1, keepdim=True)
    w = 1.0 / n
    many = (n > 1).double()
    out, a_dtemp, dtemp_terms, term_sum, a_terms, a_lse_all = {}, 0.0, 0.0, 0.0, 0.0, []
    for q, k, sname, dqn, dkn in ((c.v, c.gt, "sim_v2t", "dv", "dgt"), (c.t, c.gv, "sim_t2v", "dt", "dgv")):
        q, k = q.double(), k.double()
        sim = q @ k.t() / tc
        a_sim = 2 * U * sim.abs()
        mx = sim.amax(1, keepdim=True)
        lse = torch.logsumexp(sim, 1, keepdim=True)
        p = torch.exp(sim - lse)
        a_lse = (p * (a_sim + U * (sim - mx).abs())).sum(1, keepdim=True) + U * ((lse - mx).abs() + lse.abs() + T + 13)
        term = lse[:, 0] - (w * m * sim).sum(1)
        a_mean = (w * m * a_sim).sum(1) + U * (torch.clamp(n - 1, max=D) + 2 * many)[:, 0] * (w * m * sim.abs()).sum(1)
        a_terms = a_terms + (a_lse[:, 0] + a_mean + U * term.abs()).sum()
        term_sum = term_sum + term.abs().sum()
        r = a_sim + a_lse + U * (sim - lse).abs() + 2 * U
        ds = (p - w * m) * scale
        a_ds = r * p * scale + 4 * U * ds.abs() + TINY * (scale + 1) + U * many * w * m * scale
        out[sname] = a_sim
        out["ds" + sname[3:]] = a_ds
        ds64["ds" + sname[3:]] = ds
        a_lse_all.append(a_lse[:, 0])
        sq = (ds[:, :, None] * k[None]).cumsum(1)
        sk = (ds[:, :, None] * q[:, None, :]).cumsum(0)
        rq, rk = vc._repeats(k), vc._repeats(q)
        chain_q = torch.linalg.vector_norm(sq, dim=1) + sq[:, rq].abs().sum(1)
        chain_k = torch.linalg.vector_norm(sk, dim=0) + sk[rk].abs().sum(0)
        out[dqn] = (a_ds @ k.abs() + U * chain_q + 2 * U * (ds @ k).abs() + TINY * (G + 1)) / tc
        out[dkn] = (a_ds.t() @ q.abs() + U * chain_k + 2 * U * (ds.t() @ q).abs() + TINY * (B + 1)) / tc
        a_dtemp = a_dtemp + (a_ds * sim.abs() + ds.abs() * a_sim).sum()
        dtemp_terms = dtemp_terms + (ds * sim).abs().sum()
        out["_dtemp_" + sname] = (ds * sim).sum()
    out["lse"] = torch.cat(a_lse_all)
    loss = float(term_sum) / (2 * B)        # |loss| (every term is >= 0)
    out["loss"] = (a_terms + U * ((2 * B + 255) // 256 + 9) * term_sum) / (2 * B) + 2 * U * loss
    cnt = 2 * ((B * G + 1023) // 1024) + 22
    dtemp = (out.pop("_dtemp_sim_v2t") + out.pop("_dtemp_sim_t2v")).abs() / tc
    out["dtemp"] = (a_dtemp + U * cnt * dtemp_terms + TINY * (cnt + 1)) / tc + U * dtemp
    return out


ratios = vc.ratios


def check(c, got, ref, A, what=""):
    """Every element of every output within C * A (the constants of this module); the message names the case and the first offending element."""
    for k, (w, _) in ratios(got, ref, A).items():
        lim = C[FAMILY[k]]
        if not w <= lim:
            g, r, a = got[k].detach().cpu().double().reshape(-1), ref[k].reshape(-1), torch.as_tensor(A[k], dtype=F64).reshape(-1)
            bad = int((((g - r).abs() > lim * a) | (torch.isfinite(g) != torch.isfinite(r))).nonzero()[0])
            raise AssertionError("%s%s: %s[%d] = %r, fp64 %r, allowance %.3e = %g x A; the worst element is %.3g x A off" % (
                c.name, what, k, bad, float(g[bad]), float(r[bad]), lim * float(a[bad]), lim, w))


# ------------------------------------------------------------------------------------------------ fp32 emulator
def _emu_match(c, fault):
    ids, gids, B = c.ids, c.gids, c.B
    own = c.col0 + torch.arange(B)
    if fault == "ids32":
        low = (1 << 32) - 1
        m = ((gids[None, :] & low) == (ids[:, None] & low)) & (ids[:, None] >= 0)
    elif fault == "neg_match":
        m = gids[None, :] == ids[:, None]
    else:
        m = (gids[None, :] == ids[:, None]) & (ids[:, None] >= 0)
    if fault == "own_dropped":          # the own column counts only through its gathered id (a row left without a match keeps it)
        none = ~m.any(1)
        m[none, own[none]] = True
    else:
        m[torch.arange(B), own] = True
    return m


def emu(c, dloss=1.0, fault=None):
    """The kernels' arithmetic in fp32 torch on the CPU, in their summation orders -> dict over OUTPUTS + SAVED.  The forward, d temp and
    column parts restate vc.emu (the same kernels); the row terms and ds are the two ids kernels'.  fault: one of FAULTS."""
    B, G = c.B, c.G
    tc = vc.clamped(c.temp)
    inv = torch.tensor(1.0, dtype=F32) / tc
    half = torch.tensor(0.5, dtype=F32) / B
    q = torch.stack([c.v, c.t])                      # (2, B, E): direction 0 = v2t
    k = torch.stack([c.gt, c.gv])                    # (2, G, E)
    sim = (q.double() @ k.double().transpose(1, 2)).float() * inv          # the dot products are exact
    flat = sim.view(2 * B, G)
    mx = flat.amax(1)
    s = vc._block_sum(vc._strided_sum(torch.exp(flat - mx[:, None])))
    lse = mx + torch.log(s)
    m = _emu_match(c, fault)
    n = m.sum(1).to(F32)
    w = torch.ones((), dtype=F32) / n                # fl(1 / n_i), (B,)
    if fault == "no_div":
        w = torch.ones(B, dtype=F32)
    m2 = torch.cat([m, m])                           # the same matches in both directions, (2B, G)
    msum = wave_sum(vc._strided_sum(torch.where(m2, flat, torch.zeros(())), threads=64))      # lane l: columns l, l + 64, ...; the butterfly
    terms = lse - msum * torch.cat([w, w])
    loss = vc._block_sum(vc._strided_sum(terms[None]))[0] * half
    # backward
    scale = torch.tensor(dloss, dtype=F32) * half
    target = (m.to(F32) * w[:, None])[None]          # (1, B, G)
    ds = (torch.exp(sim - lse.view(2, B, 1)) - target) * scale
    dq = vc._fma_chain(ds.permute(2, 0, 1)[..., None], k.permute(1, 0, 2)[:, :, None, :]) * inv       # over j
    dk = vc._fma_chain(ds.permute(1, 0, 2)[..., None], q.permute(1, 0, 2)[:, :, None, :]) * inv       # over i
    cnt = B * G
    trips = (cnt + 1023) // 1024
    acc = torch.zeros(1024)
    for d in (0, 1):
        a, b = torch.zeros(trips * 1024), torch.zeros(trips * 1024)
        a[:cnt], b[:cnt] = ds[d].reshape(-1), sim[d].reshape(-1)
        a, b = a.view(trips, 1024), b.view(trips, 1024)
        for r in range(trips):
            acc = vc._fma(a[r], b[r], acc)
    wv = wave_sum(acc.view(16, 64))
    tot = torch.zeros(())
    for i in range(16):
        tot = tot + wv[i]
    dtemp = -tot / tc
    return dict(sim_v2t=sim[0], sim_t2v=sim[1], lse=lse, loss=loss, dv=dq[0], dt=dq[1], dgv=dk[1], dgt=dk[0], dtemp=dtemp, ds_v2t=ds[0], ds_t2v=ds[1])
