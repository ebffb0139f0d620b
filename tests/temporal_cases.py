"""Stress inputs, the fp64 reference and an fp64 emulation of the 16-bit kernels' roundings for the block-diagonal temporal attention (T dividing
32): attn_temporal_fwd / attn_temporal_fwd16 and their _drop twins, the grouped attn_bwd<T, 1, 1, true> and attn_temporal_bwd16, the fused
alpro_gemm_qkv_tattn and the unit form of alpro_attn_temporal_probs.  Shared by tests/test_hip_temporal_stress.py (GPU) and
tests/test_temporal_cases_cpu.py (CPU self-check); not collected itself, and nothing here touches a GPU.

One wave of those kernels holds 32 / T groups in one 32 x 32 score tile ("unit": 32 consecutive rows of one head) and only the mask
key / T == query / T keeps them apart.  mixed_groups puts a group whose scores are about N(0, 1) next to one whose scores sit near 128 (or near
94), with the cold group's queries scoring 128 (55) against the hot group's keys: a leak across the mask, or a row maximum / row sum over the tile
and not the group, is then worth whole outputs and not a few percent of one.  Every value lies on test_hip_ops.attn_inputs' grids, so the
inputs are exact in fp32, bf16 and fp16 and every q.k sum is exact in fp32.

The emulation (emu_fwd / emu_bwd) walks the same 32-row units in fp64 and rounds where the 16-bit kernels round: exp(s - max) to dt before P V,
dS and P to dt before the gradient contractions, every output to dt.  `fault=` plants one bug at a time (FWD_FAULTS / BWD_FAULTS).
"""
import torch

from tests.test_hip_ops import DOM_Q, _on_grid, attn_inputs

SCALE = 0.125
HOT = ("late_max", "offset", "early_max", "peaked")
KINDS = ("mixed",) + HOT
# (T, groups): every T dividing 32; every one but T = 32 leaves a ragged last 32-row unit, and the group counts are odd, so the last group is cold
DIAG_CASES = [(1, 37), (2, 19), (4, 11), (8, 5), (8, 13), (16, 3), (16, 5), (32, 3)]
# the grid-stride loops: fwd16 / bwd16 cap the grid at 512 workgroups of 4 waves, the fp32 forward at 2048.  With 12 heads:
MANY_UNITS_16 = (8, 700)     # 5600 rows = 175 whole chunks x 12 heads = 2100 units = 2048 + 52: a second trip that only 52 waves make
MANY_UNITS_32 = (8, 2735)    # 21880 rows: 684 chunks (the last of 24 rows) x 12 = 8208 units = 8192 + 16
MANY_H = 12
FWD_FAULTS = ("no_mask", "tile_max", "pad_last_k", "k_unit_minus_2048")
BWD_FAULTS = ("no_mask", "lse_next_head")


def units(rows, H):
    return (rows + 31) // 32 * H


def group_kind(g):
    """Even groups are cold, odd groups take the hot regimes in turn."""
    return "cold" if g % 2 == 0 else HOT[(g // 2) % 4]


def mixed_groups(T, groups, H, seed=0):
    """-> q | k | v rows (groups * T, 3 * H * 64) fp32, exact in bf16 and fp16.  Group g is built on attn_inputs' draw of its regime (one draw per
    regime, seed + i, as many groups as take that regime).  cold: the gauss draw with q[..., :4] = DOM_Q and k[..., :4] = 0 -- its own scores
    stay about N(0, 1); its queries score exactly 128 against the planted key of a late_max / early_max group (k* = (32, 32, 32, 32, 0, ...))
    and 0.125 * 4 * 8 * 13.75 = 55 plus N(0, 1) against every key of an offset group."""
    kinds = [group_kind(g) for g in range(groups)]
    t = torch.empty(groups, T, 3, H, 64)
    for i, kind in enumerate(("cold",) + HOT):
        idx = [g for g, k in enumerate(kinds) if k == kind]
        if not idx:
            continue
        part = attn_inputs(len(idx), T, H, "gauss" if kind == "cold" else kind, "none", seed + i)[0].view(len(idx), T, 3, H, 64)
        if kind == "cold":
            part[:, :, 0, :, :4] = DOM_Q
            part[:, :, 1, :, :4] = 0.0
        t[idx] = part
    return t.reshape(groups * T, 3 * H * 64).contiguous()


def inputs(kind, T, groups, H, seed=0):
    """-> (qkv (rows, 3*H*64), dout (rows, H*64)) fp32, both exact in bf16 and fp16 (dout: N(0, 1) on the 2^-5 grid)."""
    assert kind in KINDS, kind
    qkv = mixed_groups(T, groups, H, seed) if kind == "mixed" else attn_inputs(groups, T, H, kind, "none", seed)[0]
    g = torch.Generator().manual_seed(seed + 77)
    return qkv, _on_grid(torch.randn(groups * T, H * 64, generator=g), 2.0 ** -5, 7.96875)


def seed_of(kind, T, groups, H=12):
    return 3000 + 101 * T + 7 * groups + 13 * H + 1009 * KINDS.index(kind)


# ------------------------------------------------------------------------------------------------ fp64 reference
def reference(qkv, dout, T, H, keep=None):
    """fp64 on the operands as given: out (rows, H*64), lse (rows, H), and with dout the autograd gradient grad (rows, 3, H*64) of
    sum(out o dout), the softmax sm (groups, H, T, T) and the output o64 (groups, H, T, 64) the delta correction needs.  keep (groups, H, T, T):
    the dropout mask ALREADY scaled by 1 / (1 - p); lse is that of the un-dropped row."""
    rows = qkv.shape[0]
    groups = rows // T
    q64 = qkv.double().clone().requires_grad_(dout is not None)
    t = q64.view(groups, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (t[0] @ t[1].transpose(-1, -2)) * SCALE
    sm = s.softmax(-1)
    o64 = (sm if keep is None else sm * keep) @ t[2]
    out = o64.transpose(1, 2).reshape(rows, H * 64)
    res = dict(out=out.detach(), lse=torch.logsumexp(s.detach(), -1).permute(0, 2, 1).reshape(rows, H), sm=sm.detach(), o64=o64.detach())
    if dout is not None:
        out.backward(dout.double())
        res["grad"] = q64.grad.view(rows, 3, H * 64)
    return res


def excess(got, ref, rtol, atol, extra=0.0):
    """max of err / allowed (<= 1 passes); inf if got is not finite."""
    got, ref = got.detach().cpu().double(), ref.double()
    if not torch.isfinite(got).all():
        return float("inf")
    return float(((got - ref).abs() / (atol + extra + rtol * ref.abs())).max())


def grad_excess(got, ref, rtol, atol, extra=(0.0, 0.0, 0.0), mult=1.0):
    """dqkv (rows, 3*H*64) against grad (rows, 3, H*64) under test_hip_bwd_ops.check_attn_bwd's rule: atol x max(1, max|ref|) per tensor
    (x mult: 1 / (1 - p) under dropout) + extra -> [dQ, dK, dV] ratios."""
    d = got.detach().cpu().double().view(ref.shape)
    return [excess(d[:, i], ref[:, i], rtol, atol * mult * max(1.0, float(ref[:, i].abs().max())), extra[i]) for i in range(3)]


# ------------------------------------------------------------------------------------------------ emulation of the unit walk
def _rd(x, dt):
    return x.to(dt).double()


def _to_units(x, H, nsplit):
    """(rows, nsplit*H*64) -> nsplit tensors (chunks, H, 32, 64), rows past the end zero (the DMA's zero page)."""
    rows = x.shape[0]
    chunks = (rows + 31) // 32
    p = torch.zeros(chunks * 32, nsplit, H, 64, dtype=torch.float64)
    p[:rows] = x.double().view(rows, nsplit, H, 64)
    return [p[:, i].reshape(chunks, 32, H, 64).permute(0, 2, 1, 3).contiguous() for i in range(nsplit)]


def _from_units(u, rows):
    """(chunks, H, 32, 64) -> (rows, H*64)."""
    c, H = u.shape[:2]
    return u.permute(0, 2, 1, 3).reshape(c * 32, H * 64)[:rows]


def _block_mask(T):
    i = torch.arange(32) // T
    return i[:, None] == i[None, :]


def emu_fwd(qkv, T, H, dt, fault=None):
    """attn_temporal_fwd16 (dt 16-bit): per unit s = q k^T scale, the block mask, p = exp(s - rowmax) summed unrounded and rounded to dt for P V,
    out = (P V) / sum rounded to dt, lse = max + log(sum) stored in fp32.  -> out (rows, H*64), lse (rows, H), fp64 holding dt / fp32 values.
    fault: 'no_mask'; 'tile_max' (the row maximum over all 32 keys of the tile, the exponentials in fp32: a cold row beside a hot group
    underflows to 0 / 0); 'pad_last_k' (the padded key slots of the last unit hold the last valid row's K, as the fp32 forward stages them, and
    the mask lets them through); 'k_unit_minus_2048' (a wave on its second grid-stride trip still holds the K tile of its first)."""
    assert fault is None or fault in FWD_FAULTS, fault
    rows = qkv.shape[0]
    q, k, v = _to_units(qkv, H, 3)
    chunks = q.shape[0]
    allowed = _block_mask(T).expand(chunks, 1, 32, 32).clone()
    if fault == "no_mask":
        allowed[:] = True
    le = rows - (chunks - 1) * 32
    if fault == "pad_last_k" and le < 32:
        k[-1, :, le:] = k[-1, :, le - 1:le]
        allowed[-1, :, :le, le:] = True
    if fault == "k_unit_minus_2048" and chunks * H > 2048:
        ku = k.view(chunks * H, 32, 64)          # unit = chunk * H + head
        k = torch.cat([ku[:2048], ku[:chunks * H - 2048]]).view(chunks, H, 32, 64)
    s = (q @ k.transpose(-1, -2)) * SCALE
    sm = s.masked_fill(~allowed, float("-inf"))
    if fault == "tile_max":
        m = s.amax(-1, keepdim=True)
        e = torch.exp(sm - m).float().double()
    else:
        m = sm.amax(-1, keepdim=True)
        e = torch.exp(sm - m)
    tot = e.sum(-1, keepdim=True)
    out = _rd((_rd(e, dt) @ v) / tot, dt)
    lse = (m + torch.log(tot)).squeeze(-1).float().double()
    return _from_units(out, rows), lse.permute(0, 2, 1).reshape(chunks * 32, H)[:rows]


def emu_bwd(qkv, dout, lse, T, H, dt, out=None, fault=None):
    """attn_temporal_bwd16 (dt 16-bit): p = exp(s scale - lse) under the block mask, dP = dO V^T, delta = rowsum(P o dP) (out given: rowsum(dO o out),
    the fp32 kernel's form), dS = P (dP - delta) scale; dS and P rounded to dt, then dQ = dS K, dK = dS^T Q, dV = P^T dO, each rounded to dt.
    lse (rows, H).  -> (rows, 3*H*64) fp64.  fault: 'no_mask'; 'lse_next_head' (the lse rows of head h + 1)."""
    assert fault is None or fault in BWD_FAULTS, fault
    rows = qkv.shape[0]
    q, k, v = _to_units(qkv, H, 3)
    do, = _to_units(dout, H, 1)
    chunks = q.shape[0]
    lu = torch.full((chunks * 32, H), float("inf"), dtype=torch.float64)
    lu[:rows] = lse.double()
    lu = lu.view(chunks, 32, H).permute(0, 2, 1)
    if fault == "lse_next_head":
        lu = lu.roll(-1, 1)
    p = torch.exp((q @ k.transpose(-1, -2)) * SCALE - lu[..., None])
    if fault != "no_mask":
        p = p * _block_mask(T)
    dp = do @ v.transpose(-1, -2)
    delta = (p * dp).sum(-1, keepdim=True) if out is None else (do * _to_units(out, H, 1)[0]).sum(-1, keepdim=True)
    ds = _rd(p * (dp - delta) * SCALE, dt)
    pr = _rd(p, dt)
    parts = [_from_units(_rd(x, dt), rows) for x in (ds @ k, ds.transpose(-1, -2) @ q, pr.transpose(-1, -2) @ do)]
    return torch.stack([x.reshape(rows, H * 64) for x in parts], 1).reshape(rows, 3 * H * 64)
