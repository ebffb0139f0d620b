"""GPU: the video-text contrastive loss with video ids (alpro_vtc_loss_ids_fwd / _bwd and the autograd node _VtcLossIds) against the fp64
contract on the shapes, id patterns, score regimes and temperatures of tests/vtc_ids_cases.py, every element of every output within the
allowance derived there (constants measured on the CPU with an fp32 emulator, tests/test_vtc_ids_cpu.py; nothing is fitted to the kernels).
Then the relations of the contract that hold bit for bit against the plain entry points, outputs inside sentinel-guarded buffers and inputs
inside poisoned ones, the refusals, and the node's plumbing at two simulated ranks."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import vtc_cases as vc
from tests import vtc_ids_cases as ic
from tests.gemm_cases import SENTINEL, poisoned
from tests.test_hip_ops import _hip

pytestmark = pytest.mark.gpu

F32, I64 = torch.float32, torch.int64
GRAD_NAMES = ("dv", "dt", "dgv", "dgt", "dtemp")
SHAPE_ID = lambda s: "B%d_G%d_E%d_c%d" % s  # noqa: E731


def _dl(dloss):
    return torch.tensor(dloss, dtype=F32, device="cuda")


def run_ids(hip, c, dloss, ids=None, gids=None, want_dtemp=True):
    """hip.vtc_loss_ids_fwd + _bwd on the case (or on other ids) -> dict over ic.OUTPUTS."""
    v, t, gv, gt = (x.cuda() for x in (c.v, c.t, c.gv, c.gt))
    temp = c.temp.reshape(1).cuda()
    ids, gids = (c.ids if ids is None else ids).cuda(), (c.gids if gids is None else gids).cuda()
    loss, s1, s2, lse = hip.vtc_loss_ids_fwd(v, t, gv, gt, temp, ids, gids, c.col0)
    dv, dt, dgv, dgt, dtemp = hip.vtc_loss_ids_bwd(v, t, gv, gt, temp, ids, gids, c.col0, s1, s2, lse, _dl(dloss), want_dtemp=want_dtemp)
    return dict(sim_v2t=s1, sim_t2v=s2, lse=lse, loss=loss, dv=dv, dt=dt, dgv=dgv, dgt=dgt, dtemp=dtemp)


def run_plain(hip, c, dloss):
    v, t, gv, gt = (x.cuda() for x in (c.v, c.t, c.gv, c.gt))
    temp = c.temp.reshape(1).cuda()
    loss, s1, s2, lse = hip.vtc_loss_fwd(v, t, gv, gt, temp, c.col0)
    dv, dt, dgv, dgt, dtemp = hip.vtc_loss_bwd(v, t, gv, gt, temp, c.col0, s1, s2, lse, _dl(dloss))
    return dict(sim_v2t=s1, sim_t2v=s2, lse=lse, loss=loss, dv=dv, dt=dt, dgv=dgv, dgt=dgt, dtemp=dtemp)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("pattern", ic.PATTERNS)
@pytest.mark.parametrize("regime", ic.REGIMES)
@pytest.mark.parametrize("shape", ic.SHAPES, ids=SHAPE_ID)
def test_vtc_ids_against_fp64(shape, regime, pattern):
    """Both temperatures with dloss = 1.7 and, on the gauss rows, a loss-scaled backward: every element of every output within its allowance.
    One pair: the loss and every gradient are exactly 0.  (Every id equal: the rows of ds sum to 0 -- the guard test below reads ds.)"""
    hip = _hip()
    for temp in ic.TEMPS:
        c = ic.build(shape, regime, temp, pattern)
        for dloss in ic.dlosses(c):
            got = run_ids(hip, c, dloss)
            ic.check(c, got, ic.reference(c, dloss), ic.allowances(c, dloss), " dloss %g" % dloss)
            if shape[:2] == (1, 1):
                for k in ("loss",) + GRAD_NAMES:
                    assert float(got[k].abs().max()) == 0.0, "%s: %s of a single pair is not exactly 0" % (c.name, k)


# ------------------------------------------------------------------------------------------------ the contract's bitwise relations
def off_grid(shape, pattern, seed=0):
    """F.normalize(randn) rows, the own block of gv / gt equal to v / t: values whose sums round, unlike the grid's."""
    B, G, E, col0 = shape
    g = vc._gen(8100 + seed + B + G + E)
    gv, gt = (F.normalize(torch.randn(G, E, generator=g), dim=-1) for _ in range(2))
    ids, gids = ic.id_pattern(pattern, B, G, col0)
    return ic.IdCase("offgrid_B%d_G%d_E%d_c%d-%s" % (shape + (pattern,)), B, G, E, col0, "offgrid", torch.tensor(0.07), gv[col0:col0 + B].clone(),
                     gt[col0:col0 + B].clone(), gv, gt, pattern, ids, gids)


@pytest.mark.parametrize("shape", ic.SHAPES + ((64, 512, 256, 448),), ids=SHAPE_ID)
def test_vtc_ids_relations_that_hold_bit_for_bit(shape):
    hip = _hip()
    B, G, E, col0 = shape
    for build in (lambda p: off_grid(shape, p), lambda p: ic.build(shape, "dup", 0.001, p)):
        plain = None
        for pattern in ic.PATTERNS:
            c = build(pattern)
            if plain is None:
                plain = run_plain(hip, c, 1.7)
            a = run_ids(hip, c, 1.7)
            # (1) the similarities and lse are the plain entry points', whatever the ids
            for k in ("sim_v2t", "sim_t2v", "lse"):
                assert same_bits(a[k], plain[k]), "%s: %s differs from alpro_vtc_loss_fwd's" % (c.name, k)
            # (2) n_i = 1 in every row: every output is the plain entry points'
            if bool((ic.match(c.ids, c.gids, col0).sum(1) == 1).all()):
                for k in ic.OUTPUTS:
                    assert same_bits(a[k], plain[k]), "%s: %s differs from the plain entry points'" % (c.name, k)
            else:
                assert pattern not in ("distinct", "high_bits")
            # (3) two runs are equal
            b = run_ids(hip, c, 1.7)
            assert all(same_bits(a[k], b[k]) for k in ic.OUTPUTS), c.name
            # (4) without d temp the other gradients are the same
            if pattern == "dup_local":
                n = run_ids(hip, c, 1.7, want_dtemp=False)
                assert n["dtemp"] is None and all(same_bits(n[k], a[k]) for k in ("dv", "dt", "dgv", "dgt"))
        # (5) all ids negative, and negative ids against equal negative gathered ids: the plain outputs
        c = build("distinct")
        for ids, gids in ((torch.full((B,), -1, dtype=I64), torch.full((G,), -1, dtype=I64)), (torch.full((B,), -7, dtype=I64), torch.full((G,), -7, dtype=I64)),
                          (torch.full((B,), -1, dtype=I64), c.gids)):
            a = run_ids(hip, c, 1.7, ids=ids, gids=gids)
            for k in ic.OUTPUTS:
                assert same_bits(a[k], plain[k]), "%s with ids %d: %s differs from the plain entry points'" % (c.name, int(ids[0]), k)


# ------------------------------------------------------------------------------------------------ surroundings
GUARD = 3      # guard rows before and behind every view


def _inside(t, fill):
    """t (1-D or 2-D, CPU) as a contiguous view inside a `fill`ed device buffer with GUARD rows before and behind."""
    return poisoned(t.reshape(t.shape[0], -1), GUARD, 0, GUARD, fill=fill, device="cuda")


def _guards_intact(view):
    buf, R = view._base, view.shape[0]
    assert buf.shape[0] == R + 2 * GUARD
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + R:] == SENTINEL).all())


@pytest.mark.parametrize("pattern", ["dup_local", "all_equal", "negatives", "own_disagrees"])
@pytest.mark.parametrize("shape", [(5, 13, 12, 8), (130, 260, 64, 130)], ids=SHAPE_ID)
def test_vtc_ids_write_nothing_outside_their_outputs_and_read_nothing_outside_their_inputs(shape, pattern):
    """The C entry points with every output a view inside a sentinel-filled buffer, every float input inside a NaN-filled one and the id
    vectors inside buffers filled with row 0's id (a gathered id read outside the vector would be one more match): the guards keep their bits,
    every output element is written, and the results equal the wrapper's bit for bit.  The saved ds is held to its allowance, and with every
    id equal each of its rows sums to 0 within the sum of its elements' allowances."""
    hip = _hip()
    lib = hip.load()
    c = ic.build(shape, "gauss", 0.07, pattern)
    B, G, E, col0 = shape
    want = run_ids(hip, c, 1.7)
    nan = float("nan")
    v, t, gv, gt = (_inside(x, nan) for x in (c.v, c.t, c.gv, c.gt))
    tp, dl = _inside(c.temp.reshape(1), nan), _inside(torch.tensor([1.7]), nan)
    lure = int(c.ids[c.ids >= 0][0])
    ids, gids = (_inside(x, lure).reshape(-1) for x in (c.ids, c.gids))
    assert all(x.data_ptr() % 16 == 0 and x.is_contiguous() for x in (v, t, gv, gt)) and ids.is_contiguous() and ids.data_ptr() % 8 == 0
    out = {k: _inside(torch.full(s, SENTINEL), SENTINEL) for k, s in dict(
        sim_v2t=(B, G), sim_t2v=(B, G), lse=(2 * B,), loss=(1,), ds_v2t=(B, G), ds_t2v=(B, G), dv=(B, E), dt=(B, E), dgv=(G, E), dgt=(G, E), dtemp=(1,)).items()}
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.alpro_vtc_loss_ids_fwd(p(v), p(t), p(gv), p(gt), p(tp), p(ids), p(gids), B, G, E, col0, p(out["sim_v2t"]), p(out["sim_t2v"]), p(out["lse"]),
                                    p(out["loss"]), stream)
    assert rc == 0, lib.alpro_hip_last_error().decode()
    rc = lib.alpro_vtc_loss_ids_bwd(p(v), p(t), p(gv), p(gt), p(tp), p(ids), p(gids), B, G, E, col0, p(out["sim_v2t"]), p(out["sim_t2v"]), p(out["lse"]),
                                    p(dl), p(out["ds_v2t"]), p(out["ds_t2v"]), p(out["dv"]), p(out["dt"]), p(out["dgv"]), p(out["dgt"]), p(out["dtemp"]),
                                    stream)
    assert rc == 0, lib.alpro_hip_last_error().decode()
    torch.cuda.synchronize()
    for k, x in out.items():
        assert _guards_intact(x), "%s: %s wrote outside its output" % (c.name, k)
        assert bool((x != SENTINEL).all()) and bool(torch.isfinite(x).all()), "%s: %s has elements nobody wrote, or non-finite ones" % (c.name, k)
        if k in want:
            assert same_bits(x.reshape(want[k].shape), want[k]), "%s: %s differs from the wrapper's" % (c.name, k)
    ds64 = {}
    A = ic.allowances(c, 1.7, ds64)
    ic.check(c, {k: out[k] for k in ic.SAVED}, ds64, A, " (the saved ds)")
    if pattern == "all_equal":
        for k in ic.SAVED:
            rows = out[k].cpu().double().sum(1).abs()
            assert bool((rows <= ic.C["ds"] * A[k].sum(1)).all()), "%s: a row of %s sums to %.3e" % (c.name, k, float(rows.max()))


# ------------------------------------------------------------------------------------------------ refusals
ROOM = 1 << 16      # elements in every buffer handed to a call that has to refuse: were it launched all the same, it would stay inside them


def _refusal(lib, which, B, G, E, col0, null=None):
    """Calls the entry point on sentinel-filled outputs -> (return code, message, True if no output element changed)."""
    ins = [torch.zeros(ROOM, device="cuda") for _ in range(4)]
    temp, dloss = torch.full((1,), 0.07, device="cuda"), torch.ones(1, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    id_bufs = [torch.zeros(ROOM, dtype=I64, device="cuda") for _ in range(2)]
    idv = [None if null == n else p(x) for n, x in zip(("ids", "gids"), id_bufs)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if which == "fwd":
        outs = [torch.full((ROOM,), SENTINEL, device="cuda") for _ in range(4)]
        rc = lib.alpro_vtc_loss_ids_fwd(*map(p, ins), p(temp), *idv, B, G, E, col0, *map(p, outs), stream)
    else:
        saved = [torch.zeros(ROOM, device="cuda") for _ in range(3)]
        outs = [torch.full((ROOM,), SENTINEL, device="cuda") for _ in range(7)]
        rc = lib.alpro_vtc_loss_ids_bwd(*map(p, ins), p(temp), *idv, B, G, E, col0, *map(p, saved), p(dloss), *map(p, outs), stream)
    msg = lib.alpro_hip_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg, all(bool((o == SENTINEL).all()) for o in outs)


@pytest.mark.parametrize("which,B,G,E,col0,names", [
    ("fwd", 2, 4, 6, 0, "E=6"), ("fwd", 2, 4, 1028, 0, "E=1028"), ("fwd", 5, 3, 8, 0, "G=3"), ("fwd", 5, 13, 8, 9, "col0=9"), ("fwd", 5, 13, 8, -1, "col0=-1"),
    ("bwd", 2, 8193, 4, 0, "G=8193"), ("bwd", 2, 4, 6, 0, "E=6"), ("bwd", 2, 4, 1028, 0, "E=1028"), ("bwd", 5, 3, 8, 0, "G=3"),
    ("bwd", 5, 13, 8, 9, "col0=9"), ("bwd", 5, 13, 8, -1, "col0=-1")])
def test_vtc_ids_entry_points_refuse_what_the_plain_ones_refuse(which, B, G, E, col0, names):
    hip = _hip()
    rc, msg, untouched = _refusal(hip.load(), which, B, G, E, col0)
    assert rc != 0 and "alpro_vtc_loss_ids_" + which in msg and names in msg, (rc, msg)
    assert untouched, "the refused call wrote to its outputs"


@pytest.mark.parametrize("null", ["ids", "gids"])
@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_vtc_ids_entry_points_refuse_null_ids(which, null):
    hip = _hip()
    rc, msg, untouched = _refusal(hip.load(), which, 5, 13, 8, 3, null=null)
    assert rc != 0 and "alpro_vtc_loss_ids_" + which in msg and "null" in msg, (rc, msg)
    assert untouched, "the refused call wrote to its outputs"


def test_vtc_ids_wrappers_raise_on_a_refusal_and_on_wrong_id_vectors():
    hip = _hip()
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    zi = lambda n: torch.zeros(n, dtype=I64, device="cuda")  # noqa: E731
    temp = torch.full((1,), 0.07, device="cuda")
    with pytest.raises(RuntimeError, match="E=6"):
        hip.vtc_loss_ids_fwd(z(2, 6), z(2, 6), z(4, 6), z(4, 6), temp, zi(2), zi(4), 0)
    with pytest.raises(RuntimeError, match="col0=3"):
        hip.vtc_loss_ids_fwd(z(2, 8), z(2, 8), z(4, 8), z(4, 8), temp, zi(2), zi(4), 3)
    with pytest.raises(RuntimeError, match="G=8193"):
        hip.vtc_loss_ids_bwd(z(2, 4), z(2, 4), z(8193, 4), z(8193, 4), temp, zi(2), zi(8193), 0, z(2, 8193), z(2, 8193), z(4), torch.ones(1, device="cuda"))
    with pytest.raises(RuntimeError, match="int64"):         # an int32 vector would be read as half as many ids
        hip.vtc_loss_ids_fwd(z(2, 8), z(2, 8), z(4, 8), z(4, 8), temp, zi(2).int(), zi(4), 0)
    with pytest.raises(RuntimeError, match="4 elements"):    # a short gathered vector would be read past its end
        hip.vtc_loss_ids_fwd(z(2, 8), z(2, 8), z(4, 8), z(4, 8), temp, zi(2), zi(3), 0)


# ------------------------------------------------------------------------------------------------ the autograd node
NODE_B, NODE_WORLD, NODE_E = 5, 2, 12


@pytest.mark.parametrize("pattern", ["dup_local", "dup_outside"])
@pytest.mark.parametrize("rank", [0, 1])
def test_vtc_ids_autograd_node_against_fp64(rank, pattern):
    """_VtcLossIds.apply as the model calls it at rank `rank` of two: the gathered rows are torch.cat of the leaves with the other rank's
    constant rows, col0 = rank * B.  The gradient that reaches v is dv + dgv[col0 : col0 + B]; the ids receive none."""
    _hip()
    from alpro_amd.modeling.alpro_models import _VtcLossIds
    c = ic.build((NODE_B, NODE_B * NODE_WORLD, NODE_E, rank * NODE_B), "gauss", 0.07, pattern)
    assert int(ic.match(c.ids, c.gids, c.col0).sum()) > NODE_B
    lo, hi = c.col0, c.col0 + c.B
    v, t = c.v.clone().cuda().requires_grad_(True), c.t.clone().cuda().requires_grad_(True)
    temp = c.temp.clone().cuda().requires_grad_(True)
    ids, gids = c.ids.cuda(), c.gids.cuda()
    gv = torch.cat([c.gv[:lo].cuda(), v, c.gv[hi:].cuda()])
    gt = torch.cat([c.gt[:lo].cuda(), t, c.gt[hi:].cuda()])
    loss, s1, s2 = _VtcLossIds.apply(v, t, gv, gt, temp, c.col0, ids, gids)
    assert not s1.requires_grad and not s2.requires_grad and loss.requires_grad
    (loss * 1.7).backward()
    assert ids.grad is None and gids.grad is None and v.grad is not None and t.grad is not None and temp.grad.shape == temp.shape
    ref, A = ic.reference(c, 1.7), ic.allowances(c, 1.7)
    got = dict(loss=loss.detach(), sim_v2t=s1, sim_t2v=s2, dv=v.grad, dt=t.grad, dtemp=temp.grad)
    ref = dict(ref, dv=ref["dv"] + ref["dgv"][lo:hi], dt=ref["dt"] + ref["dgt"][lo:hi])
    # the sum of the two parts rounds once more
    A = dict(A, dv=A["dv"] + ic.C["dk"] / ic.C["dq"] * A["dgv"][lo:hi] + ic.U * ref["dv"].abs() / ic.C["dq"],
             dt=A["dt"] + ic.C["dk"] / ic.C["dq"] * A["dgt"][lo:hi] + ic.U * ref["dt"].abs() / ic.C["dq"])
    ic.check(c, got, ref, A, " through _VtcLossIds at rank %d" % rank)
    # a frozen temperature: no d temp, the other gradients unchanged
    v2, t2 = c.v.clone().cuda().requires_grad_(True), c.t.clone().cuda().requires_grad_(True)
    frozen = c.temp.clone().cuda()
    gv2 = torch.cat([c.gv[:lo].cuda(), v2, c.gv[hi:].cuda()])
    gt2 = torch.cat([c.gt[:lo].cuda(), t2, c.gt[hi:].cuda()])
    loss2, _, _ = _VtcLossIds.apply(v2, t2, gv2, gt2, frozen, c.col0, ids, gids)
    (loss2 * 1.7).backward()
    assert frozen.grad is None and same_bits(loss2.detach(), loss.detach()) and same_bits(v2.grad, v.grad) and same_bits(t2.grad, t.grad)
