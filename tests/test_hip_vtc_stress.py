"""GPU: the video-text contrastive loss (alpro_vtc_loss_fwd / _bwd, the five kernels of csrc/loss.hip, and the autograd node _VtcLoss the models
reach them through) against torch fp64 on the CPU, on the shapes, score regimes and temperatures of tests/vtc_cases.py.  Every element of every
output -- loss, both similarity matrices, lse, the four feature gradients, d temp -- is held to the per-element allowance derived there
(constants measured on the CPU with an fp32 emulator against fp64, tests/test_vtc_cases_cpu.py; nothing is fitted to the kernels).  Then:
outputs inside sentinel-guarded buffers and inputs inside NaN-filled ones, relations that hold bit for bit, propagation of a NaN feature to
the loss, the autograd node's plumbing, and the refusals of the two entry points."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import vtc_cases as vc
from tests.gemm_cases import SENTINEL, poisoned
from tests.test_hip_ops import _hip

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
GRAD_NAMES = ("dv", "dt", "dgv", "dgt", "dtemp")


def run(hip, c, dloss, tensors=None, want_dtemp=True, col0=None, temp=None):
    """hip.vtc_loss_fwd + hip.vtc_loss_bwd on the case's tensors (or `tensors` = (v, t, gv, gt) on the CPU) -> dict over vc.OUTPUTS."""
    v, t, gv, gt = (x.cuda() for x in (tensors or (c.v, c.t, c.gv, c.gt)))
    temp = (c.temp if temp is None else temp).reshape(1).cuda()
    col0 = c.col0 if col0 is None else col0
    loss, s1, s2, lse = hip.vtc_loss_fwd(v, t, gv, gt, temp, col0)
    dv, dt, dgv, dgt, dtemp = hip.vtc_loss_bwd(v, t, gv, gt, temp, col0, s1, s2, lse, torch.tensor(dloss, dtype=F32, device="cuda"), want_dtemp=want_dtemp)
    return dict(sim_v2t=s1, sim_t2v=s2, lse=lse, loss=loss, dv=dv, dt=dt, dgv=dgv, dgt=dgt, dtemp=dtemp)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("regime", vc.REGIMES)
@pytest.mark.parametrize("shape", vc.SHAPES, ids=lambda s: "B%d_G%d_E%d_c%d" % s)
def test_vtc_against_fp64(shape, regime):
    """Every temperature of the shape and regime with dloss = 1.7, and on the gauss rows a loss-scaled backward (dloss = 65536 * 1.7): every
    element of every output within its allowance.  One pair (B = G = 1): the loss and every gradient are exactly 0."""
    hip = _hip()
    for temp in vc.TEMPS:
        c = vc.build(shape, regime, temp)
        for dloss in ((1.7, vc.SCALED_DLOSS) if regime == "gauss" and temp in vc.SCALED_TEMPS else (1.7,)):
            got = run(hip, c, dloss)
            vc.check(c, got, vc.reference(c, dloss), vc.allowances(c, dloss), " dloss %g" % dloss)
            if shape[:2] == (1, 1):
                for k in ("loss",) + GRAD_NAMES:
                    assert float(got[k].abs().max()) == 0.0, "%s: %s of a single pair is not exactly 0" % (c.name, k)
                assert same_bits(got["lse"], torch.cat([got["sim_v2t"], got["sim_t2v"]]).reshape(2))


# ------------------------------------------------------------------------------------------------ surroundings
GUARD = 3      # guard rows before and behind every view (of E, G or 1 floats each); E % 4 == 0 keeps the key rows 16-byte aligned


def _inside(t, fill):
    """t (1-D or 2-D, CPU) as a contiguous view inside a `fill`ed device buffer with GUARD rows before and behind."""
    return poisoned(t.reshape(t.shape[0], -1), GUARD, 0, GUARD, fill=fill, device="cuda")


def _guards_intact(view):
    buf, R = view._base, view.shape[0]
    assert buf.shape[0] == R + 2 * GUARD
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + R:] == SENTINEL).all())


@pytest.mark.parametrize("regime,temp", [("gauss", 0.07), ("late_neg_last", 0.01)])
@pytest.mark.parametrize("shape", [(5, 13, 12, 8), (5, 13, 4, 3), (130, 260, 64, 130), (7, 21, 1024, 0), (3, 9, 260, 3)], ids=lambda s: "B%d_G%d_E%d_c%d" % s)
def test_vtc_writes_nothing_outside_its_outputs_and_reads_nothing_outside_its_inputs(shape, regime, temp):
    """The C entry points with every output a view inside a sentinel-filled buffer and every input inside a NaN-filled one (16-byte aligned: the
    forward reads the keys as float4): the guards keep their bits, every output element is written, and the results equal the wrapper's bit for
    bit -- a read of one element outside an input would put a NaN into them."""
    hip = _hip()
    lib = hip.load()
    c = vc.build(shape, regime, temp)
    B, G, E, col0 = shape
    want = run(hip, c, 1.7)
    nan = float("nan")
    v, t, gv, gt = (_inside(x, nan) for x in (c.v, c.t, c.gv, c.gt))
    tp, dl = _inside(c.temp.reshape(1), nan), _inside(torch.tensor([1.7]), nan)
    assert all(x.data_ptr() % 16 == 0 and x.is_contiguous() for x in (v, t, gv, gt))
    out = {k: _inside(torch.full(s, SENTINEL), SENTINEL) for k, s in dict(
        sim_v2t=(B, G), sim_t2v=(B, G), lse=(2 * B,), loss=(1,), ds_v2t=(B, G), ds_t2v=(B, G), dv=(B, E), dt=(B, E), dgv=(G, E), dgt=(G, E), dtemp=(1,)).items()}
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.alpro_vtc_loss_fwd(p(v), p(t), p(gv), p(gt), p(tp), B, G, E, col0, p(out["sim_v2t"]), p(out["sim_t2v"]), p(out["lse"]), p(out["loss"]), stream)
    assert rc == 0, lib.alpro_hip_last_error().decode()
    rc = lib.alpro_vtc_loss_bwd(p(v), p(t), p(gv), p(gt), p(tp), B, G, E, col0, p(out["sim_v2t"]), p(out["sim_t2v"]), p(out["lse"]), p(dl),
                                p(out["ds_v2t"]), p(out["ds_t2v"]), p(out["dv"]), p(out["dt"]), p(out["dgv"]), p(out["dgt"]), p(out["dtemp"]), stream)
    assert rc == 0, lib.alpro_hip_last_error().decode()
    torch.cuda.synchronize()
    for k, x in out.items():
        assert _guards_intact(x), "%s: %s wrote outside its output" % (c.name, k)
        assert bool((x != SENTINEL).all()) and bool(torch.isfinite(x).all()), "%s: %s has elements nobody wrote, or non-finite ones" % (c.name, k)
        if k in want:
            assert same_bits(x.reshape(want[k].shape), want[k]), "%s: %s differs from the wrapper's" % (c.name, k)
    ds64 = {}
    A = vc.allowances(c, 1.7, ds64)
    vc.check(c, {k: out[k] for k in vc.SAVED}, ds64, A, " (the saved ds)")


# ------------------------------------------------------------------------------------------------ exact relations
def off_grid(shape, seed=0):
    """F.normalize(randn) rows, the own block of gv / gt equal to v / t: on the grid the relations below would hold trivially."""
    B, G, E, col0 = shape
    g = vc._gen(8000 + seed + B + G + E)
    gv, gt = (F.normalize(torch.randn(G, E, generator=g), dim=-1) for _ in range(2))
    return vc.Case("offgrid_B%d_G%d_E%d_c%d" % shape, B, G, E, col0, "offgrid", torch.tensor(0.07), gv[col0:col0 + B].clone(), gt[col0:col0 + B].clone(), gv, gt)


REL_SHAPES = [(5, 13, 12, 8), (32, 32, 64, 0), (64, 512, 256, 448), (130, 260, 64, 130), (7, 21, 1024, 0)]


@pytest.mark.parametrize("shape", REL_SHAPES, ids=lambda s: "B%d_G%d_E%d_c%d" % s)
def test_vtc_relations_that_hold_bit_for_bit(shape):
    hip = _hip()
    c = off_grid(shape)
    B, G, E, col0 = shape
    a = run(hip, c, 1.7)
    # (1) v_i . t_j from either side: the same FMA chain over products that commute
    assert same_bits(a["sim_v2t"][:, col0:col0 + B], a["sim_t2v"][:, col0:col0 + B].t()), "sim_v2t's own block is not the transpose of sim_t2v's"
    # (2) a row does not depend on the rows beside it
    for i in sorted({0, B // 2, B - 1}):
        one = run(hip, c, 1.7, tensors=(c.v[i:i + 1], c.t[i:i + 1], c.gv, c.gt), col0=col0 + i)
        assert same_bits(one["sim_v2t"][0], a["sim_v2t"][i]) and same_bits(one["sim_t2v"][0], a["sim_t2v"][i]), "row %d alone has other scores" % i
        assert same_bits(one["lse"], a["lse"][[i, B + i]]), "row %d alone has another lse" % i
    # (3) exchanging the two modalities exchanges the outputs
    x = run(hip, c, 1.7, tensors=(c.t, c.v, c.gt, c.gv))
    for k, kx in (("sim_v2t", "sim_t2v"), ("sim_t2v", "sim_v2t"), ("dv", "dt"), ("dt", "dv"), ("dgv", "dgt"), ("dgt", "dgv")):
        assert same_bits(a[k], x[kx]), "%s is not %s of the exchanged call" % (k, kx)
    assert same_bits(a["lse"], torch.cat([x["lse"][B:], x["lse"][:B]]))
    for k in ("loss", "dtemp"):          # the same terms in another order of the block's sum
        p, q = float(a[k]), float(x[k])
        print("%s exchange: %s %r against %r, %.3g ulp apart" % (c.name, k, p, q, abs(p - q) / (2.0 ** -23 * max(abs(p), abs(q)))))
        assert abs(p - q) <= 2.0 ** -23 * max(abs(p), abs(q)), "%s moves by more than one fp32 rounding under the exchange: %r, %r" % (k, p, q)
    # (4) without d temp the other gradients are the same
    n = run(hip, c, 1.7, want_dtemp=False)
    assert n["dtemp"] is None and all(same_bits(n[k], a[k]) for k in ("dv", "dt", "dgv", "dgt"))
    # (5) two runs are equal
    b = run(hip, c, 1.7)
    assert all(same_bits(a[k], b[k]) for k in vc.OUTPUTS)


# ------------------------------------------------------------------------------------------------ non-finite values
@pytest.mark.parametrize("shape,row", [((5, 13, 12, 8), 2), ((64, 512, 256, 448), 300), ((130, 260, 64, 130), 257)], ids=lambda s: str(s).replace(" ", ""))
def test_vtc_carries_a_nan_feature_to_the_loss(shape, row):
    """One NaN in one gathered text row (another rank's): the loss scaler's overflow check reads the loss and the gradients.  The maximum of the
    row drops the NaN (fmaxf), the sum of exponentials has to carry it.  The NaN pattern of every output equals the fp64 reference's."""
    hip = _hip()
    c = vc.build(shape, "gauss", 0.07)
    gt = c.gt.clone()
    gt[row, shape[2] // 2] = float("nan")
    tensors = (c.v, c.t, c.gv, gt)
    got, ref = run(hip, c, 1.7, tensors=tensors), vc.reference(c, 1.7, tensors=tensors)
    assert bool(torch.isnan(ref["loss"])) and bool(torch.isnan(ref["sim_v2t"][:, row]).all()) and int(torch.isnan(ref["sim_v2t"]).sum()) == c.B
    assert bool(torch.isfinite(ref["sim_t2v"]).all()) and bool(torch.isfinite(ref["dt"]).all()) and bool(torch.isnan(ref["dv"]).all())
    for k in vc.OUTPUTS:
        g = got[k].cpu()
        assert torch.equal(torch.isnan(g), torch.isnan(ref[k])), "%s: the NaN pattern of %s differs from the reference's" % (c.name, k)
        assert not bool(torch.isinf(g).any())
    assert bool(torch.isnan(got["loss"]))
    A = {k: 2 * vc.U * ref[k].abs() for k in ("sim_v2t", "sim_t2v")}
    for k, (w, idx) in vc.ratios({k: got[k] for k in A}, ref, A).items():
        assert w <= vc.C["sim"], "%s: finite entry %d of %s is %.3g x A off" % (c.name, idx, k, w)


# ------------------------------------------------------------------------------------------------ the autograd node
NODE_B, NODE_WORLD, NODE_E = 5, 3, 12


def _node_case(rank):
    return vc.build((NODE_B, NODE_B * NODE_WORLD, NODE_E, rank * NODE_B), "gauss", 0.07)


def _node_run(c, v, t, temp, dloss=1.7):
    """_VtcLoss.apply as the model calls it: gathered rows = torch.cat of the leaves with the other ranks' constant rows."""
    from alpro_amd.modeling.alpro_models import _VtcLoss
    lo, hi = c.col0, c.col0 + c.B
    gv = torch.cat([c.gv[:lo].cuda().to(v.dtype), v, c.gv[hi:].cuda().to(v.dtype)])
    gt = torch.cat([c.gt[:lo].cuda().to(t.dtype), t, c.gt[hi:].cuda().to(t.dtype)])
    loss, s1, s2 = _VtcLoss.apply(v, t, gv, gt, temp, c.col0)
    (loss * dloss).backward()
    return loss, s1, s2


@pytest.mark.parametrize("rank", [0, NODE_WORLD - 1])
def test_vtc_autograd_node_against_fp64_autograd(rank):
    """The gradient that reaches v through the node is dv + dgv[col0 : col0 + B] (v is both the query block and a slice of the gathered keys)."""
    _hip()
    c = _node_case(rank)
    lo, hi = c.col0, c.col0 + c.B
    v, t = c.v.clone().cuda().requires_grad_(True), c.t.clone().cuda().requires_grad_(True)
    temp = c.temp.clone().cuda().requires_grad_(True)
    loss, s1, s2 = _node_run(c, v, t, temp)
    assert not s1.requires_grad and not s2.requires_grad and loss.requires_grad        # the similarity outputs are non-differentiable
    ref, A = vc.reference(c, 1.7), vc.allowances(c, 1.7)
    got = dict(loss=loss.detach(), sim_v2t=s1, sim_t2v=s2, dv=v.grad, dt=t.grad, dtemp=temp.grad)
    ref = dict(ref, dv=ref["dv"] + ref["dgv"][lo:hi], dt=ref["dt"] + ref["dgt"][lo:hi])
    # the sum of the two parts rounds once more
    A = dict(A, dv=A["dv"] + vc.C["dk"] / vc.C["dq"] * A["dgv"][lo:hi] + vc.U * ref["dv"].abs() / vc.C["dq"],
             dt=A["dt"] + vc.C["dk"] / vc.C["dq"] * A["dgt"][lo:hi] + vc.U * ref["dt"].abs() / vc.C["dq"])
    assert temp.grad.shape == temp.shape
    vc.check(c, got, ref, A, " through _VtcLoss at rank %d" % rank)
    # a frozen temperature: no d temp, the other gradients unchanged
    v2, t2 = c.v.clone().cuda().requires_grad_(True), c.t.clone().cuda().requires_grad_(True)
    frozen = c.temp.clone().cuda()
    loss2, _, _ = _node_run(c, v2, t2, frozen)
    assert frozen.grad is None and same_bits(loss2.detach(), loss.detach()) and same_bits(v2.grad, v.grad) and same_bits(t2.grad, t.grad)


def test_vtc_autograd_node_takes_bf16_and_strided_features():
    """The node's .contiguous().float(): bf16 features and strided ones give what the fp32 contiguous call on the same values gives.  The
    gathered rows are constants here, so that each leaf's gradient is one output of the backward and not a sum of two."""
    _hip()
    from alpro_amd.modeling.alpro_models import _VtcLoss
    c = _node_case(1)
    bf = torch.bfloat16
    vb, tb, gvb, gtb = (x.to(bf).cuda() for x in (c.v, c.t, c.gv, c.gt))          # (rounded off the grid: any values will do here)
    temp = c.temp.clone().cuda()

    def node(v, t, gv, gt):
        loss, s1, s2 = _VtcLoss.apply(v, t, gv, gt, temp, c.col0)
        (loss * 1.7).backward()
        return loss.detach(), s1, s2

    v0, t0 = vb.float().requires_grad_(True), tb.float().requires_grad_(True)
    base = node(v0, t0, gvb.float(), gtb.float())
    v1, t1 = vb.clone().requires_grad_(True), tb.clone().requires_grad_(True)
    low = node(v1, t1, gvb, gtb)
    assert all(same_bits(a, b) for a, b in zip(base, low)) and low[0].dtype == F32
    assert v1.grad.dtype == bf and torch.equal(v1.grad, v0.grad.to(bf)) and torch.equal(t1.grad, t0.grad.to(bf))
    wide_v, wide_t = (torch.full((c.B, 2 * c.E), float("nan"), device="cuda") for _ in range(2))
    wide_v[:, ::2], wide_t[:, ::2] = v0.detach(), t0.detach()
    v2, t2 = wide_v.requires_grad_(True), wide_t.requires_grad_(True)
    gv, gt = gvb.float().t().contiguous().t(), gtb.float().t().contiguous().t()        # the gathered rows column-major
    assert not v2[:, ::2].is_contiguous() and not gv.is_contiguous()
    strided = node(v2[:, ::2], t2[:, ::2], gv, gt)
    assert all(same_bits(a, b) for a, b in zip(base, strided))
    assert same_bits(v2.grad[:, ::2].contiguous(), v0.grad) and same_bits(t2.grad[:, ::2].contiguous(), t0.grad)
    assert float(v2.grad[:, 1::2].abs().max()) == 0.0 and float(t2.grad[:, 1::2].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ refusals
ROOM = 1 << 16      # floats in every buffer handed to a call that has to refuse: were it launched all the same, it would stay inside them


def _refusal(lib, which, B, G, E, col0):
    """Calls the entry point on sentinel-filled outputs -> (return code, message, True if no output element changed)."""
    ins = [torch.zeros(ROOM, device="cuda") for _ in range(4)]
    temp, dloss = torch.full((1,), 0.07, device="cuda"), torch.ones(1, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if which == "fwd":
        outs = [torch.full((ROOM,), SENTINEL, device="cuda") for _ in range(4)]
        rc = lib.alpro_vtc_loss_fwd(*map(p, ins), p(temp), B, G, E, col0, *map(p, outs), stream)
    else:
        saved = [torch.zeros(ROOM, device="cuda") for _ in range(3)]
        outs = [torch.full((ROOM,), SENTINEL, device="cuda") for _ in range(7)]
        rc = lib.alpro_vtc_loss_bwd(*map(p, ins), p(temp), B, G, E, col0, *map(p, saved), p(dloss), *map(p, outs), stream)
    msg = lib.alpro_hip_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg, all(bool((o == SENTINEL).all()) for o in outs)


@pytest.mark.parametrize("which,B,G,E,col0,names", [
    ("fwd", 2, 4, 6, 0, "E=6"), ("fwd", 2, 4, 1028, 0, "E=1028"), ("fwd", 5, 3, 8, 0, "G=3"), ("fwd", 5, 13, 8, 9, "col0=9"), ("fwd", 5, 13, 8, -1, "col0=-1"),
    ("bwd", 2, 8193, 4, 0, "G=8193"), ("bwd", 2, 4, 6, 0, "E=6"), ("bwd", 2, 4, 1028, 0, "E=1028"), ("bwd", 5, 3, 8, 0, "G=3"),
    ("bwd", 5, 13, 8, 9, "col0=9"), ("bwd", 5, 13, 8, -1, "col0=-1")])
def test_vtc_entry_points_refuse_what_they_cannot_run(which, B, G, E, col0, names):
    """Each refusal names the offending value and launches nothing.  The backward checks col0 as the forward does: with col0 + B > G no column
    is a positive, and it would return the gradients of another loss without a word."""
    hip = _hip()
    rc, msg, untouched = _refusal(hip.load(), which, B, G, E, col0)
    assert rc != 0 and "alpro_vtc_loss_" + which in msg and names in msg, (rc, msg)
    assert untouched, "the refused call wrote to its outputs"


def test_vtc_wrappers_raise_on_a_refusal():
    hip = _hip()
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    temp = torch.full((1,), 0.07, device="cuda")
    with pytest.raises(RuntimeError, match="E=6"):
        hip.vtc_loss_fwd(z(2, 6), z(2, 6), z(4, 6), z(4, 6), temp, 0)
    with pytest.raises(RuntimeError, match="col0=3"):
        hip.vtc_loss_fwd(z(2, 8), z(2, 8), z(4, 8), z(4, 8), temp, 3)
    with pytest.raises(RuntimeError, match="G=8193"):
        hip.vtc_loss_bwd(z(2, 4), z(2, 4), z(8193, 4), z(8193, 4), temp, 0, z(2, 8193), z(2, 8193), z(4), torch.ones(1, device="cuda"))
    with pytest.raises(RuntimeError, match="col0=3"):
        hip.vtc_loss_bwd(z(2, 8), z(2, 8), z(4, 8), z(4, 8), temp, 3, z(2, 4), z(2, 4), z(4), torch.ones(1, device="cuda"))
