"""Stress inputs, the fp64 reference, an fp32 emulator and derived allowances for the video-text contrastive loss (alpro_vtc_loss_fwd /
_bwd: the five kernels of alpro_amd/csrc/loss.hip behind _VtcLoss).  Shared by tests/test_hip_vtc_stress.py (GPU) and
tests/test_vtc_cases_cpu.py (CPU self-check); not collected itself, and nothing here touches a GPU.

Inputs.  Feature rows lie on the grid 2^-10 with |q . k| < 16, so every product is a multiple of 2^-20 and every q . k sum of up to 1024
terms is exact in fp32 in any order, with or without FMA (test_vtc_cases_cpu.py asserts fp32 matmul == fp64 matmul for every case).  The
kernel's `sim` then carries exactly two roundings, 1 / tc and the product, and the kernel and the reference see the same operands.

Reference.  Written from the model (modeling/alpro_models.py _vtc and the in-place temp.clamp_(0.001, 0.5)), not from the kernel, in
fp64: tc = clamp(temp, 0.001, 0.5) taken in fp32 as the parameter is, sim = q k^T / tc, loss = (mean_i ce_v2t[i] + mean_i ce_t2v[i]) / 2
with ce[i] = logsumexp(sim[i]) - sim[i, col0 + i]; gradients by autograd with tc as the leaf of d temp (what clamp_ in place leaves the
optimizer with), so d temp is checked at the clamped temperatures too.

Allowances, u = 2^-24; first order in u, every quantity on the right from fp64; nothing is fitted to a kernel's output.  Per direction,
with p = exp(sim - lse), scale = dloss / (2B), ds = (p - [j == col0 + i]) * scale, mx = max_j sim, T = ceil(G / 256):
  sim    fl(acc * fl(1 / tc)), acc exact:                                   A_sim = 2 u |sim|
  lse    fl(mx + logf(s)), s = sum_j expf(fl(sim_j - mx)).  lse is a p-weighted mean of its inputs' errors; the exp arguments round by
         u |sim_j - mx|; expf and logf a constant number of ulps (2 each here); the sum passes T + 9 additions (T trips per thread, six
         butterfly steps, three wave adds) of terms that are all positive, so its relative error is at most (T + 9) u; the last add
         rounds by u |lse|:
                 A_lse = sum_j p_j (A_sim_j + u |sim_j - mx|) + u (|log s| + |lse| + T + 13)
  loss   2B terms lse - sim_pos (each rounds by u |term|), at most ceil(2B / 256) + 9 additions deep, times fl(0.5 / B):
                 A_loss = [sum_k (A_lse_k + A_sim_pos_k + u |term_k|) + u (ceil(2B / 256) + 9) sum_k |term_k|] / (2B) + 2 u |loss|
  p      expf(fl(sim - lse)):  relative  r = A_sim + A_lse + u |sim - lse| + 2 u   (|sim| + |lse| in units of u, plus a few ulps)
  ds     (p - 1 is exact or rounds by u |p - 1|; scale = fl(dloss * fl(0.5 / B)); one more multiply; below 2^-126 fp32 flushes or
         loses bits where fp64 still holds 1e-200):                         A_ds = r p |scale| + 4 u |ds| + 2^-126 (|scale| + 1)
  dq     d query i = fl(S_G * fl(1 / tc)), S_k = fmaf(ds_ik, key_k, S_{k-1}): G addends one after the other, one rounding each, so
         the chain's error is sum_k d_k S_k with |d_k| <= u.  Its worst case u sum_k |S_k| is 1.8e-4 of the largest gradient on the
         `gauss` rows at G = 8192 before any constant (and the looser u G sum_j |ds_ij key_j| is 5.9e-4), although the emulator is within
         1.4e-6 there: either would open the allowance where the problem is benign.  So the d_k count as independent and of mean
         zero (the probabilistic model of Higham & Mary 2019: the root sum of squares takes the place of the sum), EXCEPT at a step
         whose key row repeats an earlier one bit for bit -- the `dup` rows add the same addend thousands of times, the roundings
         drift in one direction (the emulator was 5.2 root sums of squares off on dup at G = 8192), and those steps enter at their
         worst case:
                 chain = sqrt(sum_k S_k^2) + sum_{k repeats} |S_k|
                 A_dq = (sum_j A_ds_ij |key_j| + u chain + 2 u |S_G| + (G + 1) 2^-126) / tc
  dk     d key j = the same chain over the B queries i (repeats: query rows equal to an earlier one)
  dtemp  -sum ds sim / tc over both directions: 1024 threads, 2 ceil(BG / 1024) FMAs each, six butterfly steps, sixteen wave adds:
                 A_dtemp = (sum (A_ds |sim| + |ds| A_sim) + u n sum |ds sim| + (n + 1) 2^-126) / tc + u |dtemp|,   n = 2 ceil(BG / 1024) + 22
The allowance of an output is C * A.  C is measured, not chosen: the largest error / A of the fault-free emulator below (emu) against
the fp64 reference over every case (MEASURED, re-measured by tests/test_vtc_cases_cpu.py on every run), times MARGIN = 4 for what the CPU
need not reproduce: the device's expf / logf differing from the host's by an ulp or two, the wave-tree order of the block reductions, FMA
contraction.

Conditioning, measured here with the emulator (plain fp32 in the kernels' order) against fp64, so a later change has the numbers:
  * offset_pos / offset_neg at tc = 0.001: |sim| is about 1000 everywhere and sum ds * sim cancels against it; the emulator's d temp is
    off by 2 % of its value at (3, 3, 256), 0.2 - 0.6 % at the other small shapes and 0.004 - 0.1 % at the large ones, where d temp of
    a benign case is good to 1e-7 (test_vtc_cases_cpu.py prints the table); the allowance there is 2.4 - 14 % of d temp.  The better-
    conditioned form sum ds * (sim - mx) is deliberately NOT what the kernel or the emulator computes.
  * aligned at tc <= 0.01: p_pos - 1 cancels completely (fp32: exactly 0; fp64: 1e-30 and below); the gradients' error exceeds their
    magnitude, and A_ds = r p |scale| with r about 1e-4 is what bounds them.
  * gauss at temp = 0.07: every gradient's allowance is at most 4.4e-5 of the output's largest magnitude (asserted below 1e-4; the one
    pair aside, whose outputs are exactly 0), the emulator's own error 3e-8 .. 1.4e-6 of it.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from tests.rowwise_cases import U24, _gen, on_grid, wave_sum

F32, F64 = torch.float32, torch.float64
U = U24
STEP = 2.0 ** -10
TINY = 2.0 ** -126         # below it fp32 flushes or loses bits; fp64 does not
T_LO, T_HI = 0.001, 0.5

# (B, G, E, col0)
SHAPES = (
    (1, 1, 256, 0),            # loss and every gradient exactly 0
    (3, 3, 256, 0),
    (5, 13, 12, 8),            # G no multiple of B, col0 + B = G, E < 256
    (5, 13, 4, 3),             # smallest E, col0 no multiple of B
    (3, 9, 260, 3),            # E > 256 with E % 256 != 0
    (64, 512, 256, 448),       # the workload's shape, last rank
    (130, 260, 64, 130),       # 2B = 260: second trip of the finish kernel; G = 260: a 4-column second trip
    (16, 8192, 32, 8176),      # the backward's largest G
    (7, 21, 1024, 0),          # largest E: four trips of the q load and the e loops
)
REGIMES = ("gauss", "aligned", "offset_pos", "offset_neg", "dup", "late_neg_last", "late_neg_first")
TEMPS = (0.07, 0.01, 0.001, 0.0001, 0.5, 0.9)     # initial value; small; the bounds exactly; clamped up; clamped down
SCALED_DLOSS, SCALED_TEMPS = 65536 * 1.7, (0.07, 0.001)     # the loss-scaled backward: on the gauss rows at these temperatures
OUTPUTS = ("sim_v2t", "sim_t2v", "lse", "loss", "dv", "dt", "dgv", "dgt", "dtemp")     # what the wrappers return
SAVED = ("ds_v2t", "ds_t2v")        # what the backward's C entry point also writes: the rows kernel's ds, kept for the columns kernel
FAULTS = ("no_max", "max_first256", "pos_at_i", "no_clamp", "inv_b", "dtemp_one_dir", "swap_dg", "loss_first256", "dq_no_tc")

# Largest error / A of the fault-free emulator against fp64 over SHAPES x REGIMES x TEMPS with dloss = 1.7 and, on gauss at SCALED_TEMPS,
# with SCALED_DLOSS (tests/test_vtc_cases_cpu.py::test_emulator_stays_within_a_quarter_of_every_constant re-measures and prints them), and
# the constants: MARGIN x the measured value rounded up by about a tenth (a host whose expf / logf round another way moves the figures by
# a few per cent).  Keys: the families of outputs that share a derivation.  Worst cases: sim (16, 8192, 32) gauss 0.01; lse (5, 13, 12)
# dup 0.001; loss (5, 13, 4) late_neg_last 0.001; ds (3, 9, 260) gauss 0.01; dq and dk (130, 260, 64) late_neg_first 0.07; dtemp
# (3, 9, 260) aligned 0.5.
MARGIN = 4.0
MEASURED = {"sim": 0.6874, "lse": 0.6244, "loss": 0.0962, "ds": 0.6216, "dq": 0.8147, "dk": 1.2326, "dtemp": 0.0702}
RECORDED = {"sim": 0.75, "lse": 0.7, "loss": 0.11, "ds": 0.7, "dq": 0.9, "dk": 1.4, "dtemp": 0.08}       # MEASURED rounded up by about a tenth
C = {k: MARGIN * m for k, m in RECORDED.items()}       # sim 3, lse 2.8, loss 0.44, ds 2.8, dq 3.6, dk 5.6, dtemp 0.32
FAMILY = {"sim_v2t": "sim", "sim_t2v": "sim", "lse": "lse", "loss": "loss", "dv": "dq", "dt": "dq", "dgv": "dk", "dgt": "dk", "dtemp": "dtemp",
          "ds_v2t": "ds", "ds_t2v": "ds"}

Case = namedtuple("Case", "name B G E col0 regime temp v t gv gt")


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def late_col(regime, G):
    return G - 1 if regime == "late_neg_last" else 0


def build(shape, regime, temp, seed=0):
    """-> Case: gathered rows gv, gt (G, E) of the regime on the 2^-10 grid, the rank's own rows v, t = rows col0 .. col0 + B of them (what
    allgather hands the model), temp a 0-d fp32 tensor."""
    B, G, E, col0 = shape
    g = _gen(7000 + seed + 31 * B + 7 * G + E + col0 + 1000 * REGIMES.index(regime))
    z1, z2 = torch.randn(G, E, generator=g), torch.randn(G, E, generator=g)
    w = on_grid(_unit(torch.randn(E, generator=g)), STEP)
    jit = lambda lim: torch.randint(-lim, lim + 1, (G, E), generator=g).float() * STEP  # noqa: E731  (a few grid steps)
    if regime in ("gauss", "dup"):
        gv, gt = on_grid(z1 / math.sqrt(E), STEP), on_grid(z2 / math.sqrt(E), STEP)
        if regime == "dup":          # rows 0, 3, 6, ... identical: ties in every row, and the positives among them have copies
            gv[0::3], gt[0::3] = gv[0].clone(), gt[0].clone()
    elif regime == "aligned":        # t_j = v_j up to two grid steps, unit rows: the positive is the largest score of its row
        gv = on_grid(_unit(z1), STEP)
        gt = gv + jit(2)
    elif regime in ("offset_pos", "offset_neg"):     # every row within three grid steps of +w (gv) and of +-w (gt), |w| = 1
        gv = w + jit(3)
        gt = (w if regime == "offset_pos" else -w) + jit(3)
    elif regime in ("late_neg_last", "late_neg_first"):
        # every row within cos 0.94 of w (|z + 3w| rows, unit length), the key of one column 2w: its score is >= 1.88 / tc in every row, a
        # positive's at most 1 / tc
        gv, gt = on_grid(_unit(_unit(z1) + 3 * w), STEP), on_grid(_unit(_unit(z2) + 3 * w), STEP)
        c = late_col(regime, G)
        gv[c], gt[c] = 2 * w, 2 * w
    else:
        raise ValueError(regime)
    gv, gt = gv.contiguous(), gt.contiguous()
    assert gv.dtype == F32 and float(gv.abs().max()) <= 4
    name = "B%d_G%d_E%d_c%d-%s-t%g" % (B, G, E, col0, regime, temp)
    return Case(name, B, G, E, col0, regime, torch.tensor(temp, dtype=F32), gv[col0:col0 + B].clone(), gt[col0:col0 + B].clone(), gv, gt)


def cases(shapes=SHAPES, regimes=REGIMES, temps=TEMPS):
    for s in shapes:
        for r in regimes:
            for t in temps:
                yield build(s, r, t)


def clamped(temp):
    """tc as the model's in-place clamp_ leaves the fp32 parameter."""
    return temp.to(F32).clamp(T_LO, T_HI)


# ------------------------------------------------------------------------------------------------ fp64 reference
def _loss64(v, t, gv, gt, tc, col0):
    B = v.shape[0]
    sv, st = v @ gt.t() / tc, t @ gv.t() / tc
    pos = torch.arange(B)
    lv, lt = torch.logsumexp(sv, 1), torch.logsumexp(st, 1)
    loss = ((lv - sv[pos, col0 + pos]).mean() + (lt - st[pos, col0 + pos]).mean()) / 2
    return loss, sv, st, torch.cat([lv, lt])


def reference(c, dloss=1.0, tensors=None):
    """fp64 -> dict over OUTPUTS (gradients of dloss * loss; dtemp with respect to the clamped temperature).  tensors: (v, t, gv, gt) in
    place of the case's (the non-finite test)."""
    v, t, gv, gt = (x.double().requires_grad_(True) for x in (tensors or (c.v, c.t, c.gv, c.gt)))
    tc = clamped(c.temp).double().requires_grad_(True)
    loss, sv, st, lse = _loss64(v, t, gv, gt, tc, c.col0)
    (loss * dloss).backward()
    return dict(sim_v2t=sv.detach(), sim_t2v=st.detach(), lse=lse.detach(), loss=loss.detach(), dv=v.grad, dt=t.grad, dgv=gv.grad, dgt=gt.grad,
                dtemp=tc.grad)


# ------------------------------------------------------------------------------------------------ allowances
def allowances(c, dloss=1.0, ds64=None):
    """fp64 -> dict over OUTPUTS + SAVED of A (the module docstring), before the constant.  ds64: a dict that receives the fp64 ds_v2t / ds_t2v."""
    ds64 = {} if ds64 is None else ds64
    B, G, col0 = c.B, c.G, c.col0
    tc = float(clamped(c.temp))
    T = (G + 255) // 256
    scale = abs(dloss) / (2 * B)
    pos = torch.arange(B)
    out, a_dtemp, dtemp_terms, term_sum, a_terms, a_lse_all = {}, 0.0, 0.0, 0.0, 0.0, []
    for q, k, sname, dqn, dkn in ((c.v, c.gt, "sim_v2t", "dv", "dgt"), (c.t, c.gv, "sim_t2v", "dt", "dgv")):
        q, k = q.double(), k.double()
        sim = q @ k.t() / tc
        a_sim = 2 * U * sim.abs()
        mx = sim.amax(1, keepdim=True)
        lse = torch.logsumexp(sim, 1, keepdim=True)
        p = torch.exp(sim - lse)
        a_lse = (p * (a_sim + U * (sim - mx).abs())).sum(1, keepdim=True) + U * ((lse - mx).abs() + lse.abs() + T + 13)
        term = (lse[:, 0] - sim[pos, col0 + pos])
        a_terms = a_terms + (a_lse[:, 0] + a_sim[pos, col0 + pos] + U * term.abs()).sum()
        term_sum = term_sum + term.abs().sum()
        r = a_sim + a_lse + U * (sim - lse).abs() + 2 * U
        onehot = torch.zeros_like(sim)
        onehot[pos, col0 + pos] = 1.0
        ds = (p - onehot) * scale
        a_ds = r * p * scale + 4 * U * ds.abs() + TINY * (scale + 1)
        out[sname] = a_sim
        out["ds" + sname[3:]] = a_ds
        ds64["ds" + sname[3:]] = ds
        a_lse_all.append(a_lse[:, 0])
        sq = (ds[:, :, None] * k[None]).cumsum(1)              # partial sums of the rows kernel's chain over j, (B, G, E)
        sk = (ds[:, :, None] * q[:, None, :]).cumsum(0)        # ... of the columns kernel's chain over i
        rq, rk = _repeats(k), _repeats(q)
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
    n = 2 * ((B * G + 1023) // 1024) + 22
    dtemp = (out.pop("_dtemp_sim_v2t") + out.pop("_dtemp_sim_t2v")).abs() / tc
    out["dtemp"] = (a_dtemp + U * n * dtemp_terms + TINY * (n + 1)) / tc + U * dtemp
    return out


def _repeats(x):
    """(n, E) -> bool (n,): the row equals an earlier row bit for bit."""
    n = x.shape[0]
    _, inv = torch.unique(x, dim=0, return_inverse=True)
    first = torch.full((int(inv.max()) + 1,), n, dtype=torch.int64).scatter_reduce(0, inv, torch.arange(n), "amin")
    return torch.arange(n) != first[inv]


def ratios(got, ref, A):
    """-> {output: (worst error / A, flat index of the first element that far off)}.  inf where one of got / ref is finite and the other is
    not, or where A is 0 and the error is not; elements non-finite on both sides count as 0 (their pattern is the caller's to compare)."""
    res = {}
    for k in OUTPUTS + SAVED:
        if got.get(k) is None or k not in ref:
            continue
        g, r, a = got[k].detach().cpu().double().reshape(-1), ref[k].reshape(-1), torch.as_tensor(A[k], dtype=F64).reshape(-1)
        both = torch.isfinite(g) & torch.isfinite(r)
        err = torch.where(both, (g - r).abs(), torch.zeros_like(r))
        ratio = torch.where(err == 0, torch.zeros_like(err), err / a)
        ratio = torch.where(torch.isfinite(g) != torch.isfinite(r), torch.full_like(ratio, float("inf")), ratio)
        w = float(ratio.max())
        res[k] = (w, int((ratio == w).nonzero()[0]))
    return res


def check(c, got, ref, A, what=""):
    """Every element of every output within C * A; the message names the case, the output and the first offending element."""
    for k, (w, _) in ratios(got, ref, A).items():
        lim = C[FAMILY[k]]
        if not w <= lim:
            g, r, a = got[k].detach().cpu().double().reshape(-1), ref[k].reshape(-1), torch.as_tensor(A[k], dtype=F64).reshape(-1)
            bad = int((((g - r).abs() > lim * a) | (torch.isfinite(g) != torch.isfinite(r))).nonzero()[0])
            raise AssertionError("%s%s: %s[%d] = %r, fp64 %r, allowance %.3e = %g x A; the worst element is %.3g x A off" % (
                c.name, what, k, bad, float(g[bad]), float(r[bad]), lim * float(a[bad]), lim, w))


# ------------------------------------------------------------------------------------------------ fp32 emulator
def _fma(a, b, acc):
    """fmaf in fp32: the product is exact in fp64, the sum is rounded to fp64 and then to fp32."""
    return (a.double() * b.double() + acc.double()).float()


def _fma_chain(a, b):
    """acc = fmaf(a[n], b[n], acc) for n = 0, 1, ... in fp32 (broadcasting a[n] against b[n]); numpy, for the 8192 steps of the longest chain."""
    a, b = a.double().contiguous(), b.double().contiguous()
    shape = torch.broadcast_shapes(a.shape[1:], b.shape[1:])
    if math.prod(shape) > 4096:          # few long steps: torch's threads; many short ones: numpy's smaller cost per call
        acc = torch.zeros(shape, dtype=F64)
        for n in range(a.shape[0]):
            acc = (a[n] * b[n] + acc).float().double()
        return acc.float()
    a, b = a.numpy(), b.numpy()
    acc = np.zeros(shape, dtype=np.float64)
    for n in range(a.shape[0]):
        acc = (a[n] * b[n] + acc).astype(np.float32).astype(np.float64)
    return torch.from_numpy(acc.astype(np.float32))


def _block_sum(x):
    """loss.hip block_reduce of per-thread values (R, 256): wave butterflies, then waves 0..3 in order."""
    w = wave_sum(x.view(-1, 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def _strided_sum(x, threads=256):
    """(R, n) -> (R, threads): thread k adds elements k, k + threads, ... in ascending order."""
    R, n = x.shape
    trips = (n + threads - 1) // threads
    pad = torch.zeros(R, trips * threads, dtype=F32)
    pad[:, :n] = x
    pad = pad.view(R, trips, threads)
    s = torch.zeros(R, threads, dtype=F32)
    for k in range(trips):
        s = s + pad[:, k]
    return s


def emu(c, dloss=1.0, fault=None):
    """The five kernels' arithmetic in fp32 torch on the CPU, in their summation orders -> dict over OUTPUTS.  fault: one of FAULTS."""
    B, G, E, col0 = c.B, c.G, c.E, c.col0
    tc = c.temp.to(F32) if fault == "no_clamp" else clamped(c.temp)
    inv = torch.tensor(1.0, dtype=F32) / tc
    half = torch.tensor(1.0 if fault == "inv_b" else 0.5, dtype=F32) / B
    pos = torch.arange(B)
    pcol = pos if fault == "pos_at_i" else col0 + pos
    q = torch.stack([c.v, c.t])                      # (2, B, E): direction 0 = v2t
    k = torch.stack([c.gt, c.gv])                    # (2, G, E)
    sim = (q.double() @ k.double().transpose(1, 2)).float() * inv          # the dot products are exact
    flat = sim.view(2 * B, G)
    if fault == "no_max":
        mx = torch.zeros(2 * B)
    elif fault == "max_first256":
        mx = flat[:, :256].amax(1)
    else:
        mx = flat.amax(1)
    s = _block_sum(_strided_sum(torch.exp(flat - mx[:, None])))
    lse = mx + torch.log(s)
    terms = lse - torch.cat([sim[0][pos, pcol], sim[1][pos, pcol]])
    if fault == "loss_first256":
        terms = terms[:256]
    loss = _block_sum(_strided_sum(terms[None]))[0] * half
    # backward
    scale = torch.tensor(dloss, dtype=F32) * half
    onehot = torch.zeros(2, B, G)
    onehot[:, pos, pcol] = 1.0
    ds = (torch.exp(sim - lse.view(2, B, 1)) - onehot) * scale
    dq = _fma_chain(ds.permute(2, 0, 1)[..., None], k.permute(1, 0, 2)[:, :, None, :])        # over j: (2, B, 1) x (2, 1, E)
    if fault != "dq_no_tc":
        dq = dq * inv
    dk = _fma_chain(ds.permute(1, 0, 2)[..., None], q.permute(1, 0, 2)[:, :, None, :]) * inv    # over i: (2, G, 1) x (2, 1, E)
    n = B * G
    trips = (n + 1023) // 1024
    acc = torch.zeros(1024)
    for d in ((0,) if fault == "dtemp_one_dir" else (0, 1)):
        a, b = torch.zeros(trips * 1024), torch.zeros(trips * 1024)
        a[:n], b[:n] = ds[d].reshape(-1), sim[d].reshape(-1)
        a, b = a.view(trips, 1024), b.view(trips, 1024)
        for r in range(trips):
            acc = _fma(a[r], b[r], acc)
    w = wave_sum(acc.view(16, 64))
    tot = torch.zeros(())
    for i in range(16):
        tot = tot + w[i]
    dtemp = -tot / tc
    dgt, dgv = dk[0], dk[1]
    if fault == "swap_dg":
        dgt, dgv = dgv, dgt
    return dict(sim_v2t=sim[0], sim_t2v=sim[1], lse=lse, loss=loss, dv=dq[0], dt=dq[1], dgv=dgv, dgt=dgt, dtemp=dtemp, ds_v2t=ds[0], ds_t2v=ds[1])
