"""CPU: the self-check of tests/vtc_ids_cases.py (the fp64 reference with distinct ids is vc.reference, the fault-free emulator of the ids
kernels stays within a quarter of every recorded constant -- that is where the constants come from -- and every planted fault exceeds an
allowance), the hard-negative sampler that respects video ids (AlproBaseModel._sample_negatives_ids) on CPU tensors, input_gpu.video_ids, the
declarations of the two entry points, and dist.allgather of an int64 vector at world size 2 over gloo.

Which of these need the feature: the sampler tests, video_ids and the declarations fail without it.  The emulator, reference, pattern, row-sum and
planted-fault tests check tests/vtc_ids_cases.py itself, and the gloo test pins a property dist.allgather already had (an integer tensor comes
back without grad_fn); they pass with or without the kernels and are there so that the allowances and that property cannot drift unnoticed."""
import functools
import hashlib
import os
import re
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

from tests import vtc_cases as vc
from tests import vtc_ids_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = torch.int64


# ------------------------------------------------------------------------------------------------ the cases, the reference, the emulator
@functools.lru_cache(maxsize=None)
def _sweep():
    """One pass over every case and dloss: reference, allowances and the fault-free emulator -> list of (case name, pattern, dloss, {output:
    error / A})."""
    rows = []
    for c in ic.cases():
        for dl in ic.dlosses(c):
            ds64 = {}
            ref, A, got = ic.reference(c, dl), ic.allowances(c, dl, ds64), ic.emu(c, dl)
            ref.update(ds64)
            rows.append((c.name, c.pattern, dl, {k: w for k, (w, _) in ic.ratios(got, ref, A).items()}))
    return rows


def test_emulator_stays_within_a_quarter_of_every_constant():
    """Re-measures ic.MEASURED: the worst error / A of the fault-free emulator per family of outputs over every case.  Above C / 4 the margin
    is gone; below C / 8 the recorded constant is stale and has to be measured again."""
    rows = _sweep()
    assert len(rows) == len(ic.SHAPES) * len(ic.PATTERNS) * len(ic.TEMPS) * (len(ic.REGIMES) + 1)       # gauss twice: dloss 1.7 and loss-scaled
    worst = {}
    for name, _, dl, ratios in rows:
        for k, w in ratios.items():
            f = ic.FAMILY[k]
            if w > worst.get(f, (-1.0, ""))[0]:
                worst[f] = (w, "%s %s dloss %g" % (name, k, dl))
    print()
    for f, (w, where) in worst.items():
        print("[vtc ids allowance] %-5s emulator / A %.4f (recorded %.4f, constant %.2f) at %s" % (f, w, ic.MEASURED[f], ic.C[f], where))
    assert set(worst) == set(ic.C) and ic.MARGIN == vc.MARGIN == 4.0
    for f, (w, where) in worst.items():
        assert ic.C[f] == ic.MARGIN * ic.RECORDED[f] and ic.MEASURED[f] <= ic.RECORDED[f]
        assert w <= ic.C[f] / 4, "%s: emulator at %.3f x A (%s), the constant %.3f leaves less than the margin of 4" % (f, w, where, ic.C[f])
        assert w >= ic.C[f] / 8, "%s: emulator at most %.3f x A, the constant %.3f is stale" % (f, w, ic.C[f])


def test_reference_with_distinct_ids_is_the_plain_reference():
    """n_i = 1: the contract's loss is the plain loss, in fp64 to the last bit of every output but the gradients' (another graph: 1e-15), and
    the ids' allowances are vc's.  All ids negative: the same."""
    for shape in ic.SHAPES[:5]:
        for regime in ic.REGIMES:
            c = ic.build(shape, regime, 0.07, "distinct")
            none = c._replace(ids=torch.full_like(c.ids, -1), gids=torch.full_like(c.gids, -1))
            plain, A_plain = vc.reference(c, 1.7), vc.allowances(c, 1.7)
            for cc in (c, none):
                ref, A = ic.reference(cc, 1.7), ic.allowances(cc, 1.7)
                for k in ic.OUTPUTS:
                    top = float(plain[k].abs().max())
                    assert float((ref[k] - plain[k]).abs().max()) <= 1e-13 * max(top, 1.0), (c.name, k)
                for k in ic.OUTPUTS + ic.SAVED:
                    assert torch.allclose(torch.as_tensor(A[k]), torch.as_tensor(A_plain[k]), rtol=1e-12, atol=0), (c.name, k)


def test_patterns_do_what_they_claim():
    for B, G, _, col0 in ic.SHAPES:
        own = col0 + torch.arange(B)
        n = {p: ic.match(*ic.id_pattern(p, B, G, col0), col0).sum(1) for p in ic.PATTERNS}
        for p in ic.PATTERNS:
            ids, gids = ic.id_pattern(p, B, G, col0)
            assert ids.dtype == I64 and gids.dtype == I64 and ids.shape == (B,) and gids.shape == (G,)
            assert bool(ic.match(ids, gids, col0)[torch.arange(B), own].all())
        assert bool((n["distinct"] == 1).all()) and bool((n["all_equal"] == G).all()) and bool((n["high_bits"] == 1).all())
        ids, gids = ic.id_pattern("negatives", B, G, col0)
        assert bool((ids[0::2] == -1).all()) and bool((n["negatives"][0::2] == 1).all()) and int((gids == -1).sum()) >= (2 if G >= 4 else 1)
        ids, gids = ic.id_pattern("high_bits", B, G, col0)
        assert B < 2 or (ids[0] != ids[1] and (ids[0] & 0xFFFFFFFF) == (ids[1] & 0xFFFFFFFF))
        ids, gids = ic.id_pattern("own_disagrees", B, G, col0)
        assert gids[col0] != ids[0] and (G == B or n["own_disagrees"][0] == 2)
        if B >= 2:
            assert n["dup_local"][0] == 2 and n["dup_local"][1] == 2
        if G > B:
            ids, gids = ic.id_pattern("dup_outside", B, G, col0)
            assert n["dup_outside"][0] >= 2 and len(set(gids[own].tolist())) == B        # a copy outside the own block, none inside
        if (B, G) == (130, 260):
            assert int(own.max()) >= 256        # matches behind column 255


def test_every_row_of_ds_sums_to_zero_when_every_id_is_equal():
    """n_i = G: softmax minus the uniform target.  The emulator's rows sum to 0 within the sum of their elements' allowances."""
    for shape in ((3, 3, 256, 0), (5, 13, 12, 8), (130, 260, 64, 130)):
        c = ic.build(shape, "gauss", 0.07, "all_equal")
        A, got = ic.allowances(c, 1.7), ic.emu(c, 1.7)
        for k in ic.SAVED:
            assert bool((got[k].double().sum(1).abs() <= ic.C["ds"] * A[k].sum(1)).all()), (c.name, k)


# fault -> (shape, regime, temp, pattern, the output whose allowance it exceeds there)
FAULT_CASES = {
    "no_div": ((3, 3, 256, 0), "gauss", 0.07, "all_equal", "loss"),
    "own_dropped": ((5, 13, 12, 8), "gauss", 0.07, "own_disagrees", "loss"),
    "ids32": ((5, 13, 12, 8), "gauss", 0.07, "high_bits", "loss"),
    "neg_match": ((5, 13, 4, 3), "gauss", 0.07, "negatives", "loss"),
}
FAULT_CASES_DS = {       # the same faults seen by the backward alone
    "no_div": ((5, 13, 12, 8), "gauss", 0.07, "dup_local", "ds_v2t"),
    "own_dropped": ((5, 13, 4, 3), "gauss", 0.07, "own_disagrees", "dv"),
    "ids32": ((130, 260, 64, 130), "gauss", 0.07, "high_bits", "ds_t2v"),
    "neg_match": ((130, 260, 64, 130), "gauss", 0.07, "negatives", "dgv"),
}


@pytest.mark.parametrize("table", [FAULT_CASES, FAULT_CASES_DS], ids=["loss", "backward"])
def test_every_planted_fault_exceeds_an_allowance(table):
    assert set(table) == set(ic.FAULTS)
    for fault, (shape, regime, temp, pattern, out) in table.items():
        c = ic.build(shape, regime, temp, pattern)
        ds64 = {}
        ref, A = ic.reference(c, 1.7), ic.allowances(c, 1.7, ds64)
        ref.update(ds64)
        clean = ic.ratios(ic.emu(c, 1.7), ref, A)
        assert all(w <= ic.C[ic.FAMILY[k]] / 4 for k, (w, _) in clean.items()), (fault, clean)
        bad = ic.ratios(ic.emu(c, 1.7, fault=fault), ref, A)
        print("[vtc ids fault] %-12s on %s: %s at %.3g x A (constant %.2f)" % (fault, c.name, out, bad[out][0], ic.C[ic.FAMILY[out]]))
        assert bad[out][0] > ic.C[ic.FAMILY[out]], "%s passes on %s: %s at %.3g x A" % (fault, c.name, out, bad[out][0])
        with pytest.raises(AssertionError, match=re.escape(c.name)):
            ic.check(c, ic.emu(c, 1.7, fault=fault), ref, A)


# ------------------------------------------------------------------------------------------------ the sampler
def _sims(bs, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(bs, bs, generator=g) * 2.0, torch.randn(bs, bs, generator=g) * 2.0


def _mask(ids):
    """The mask the issue states, restated: same non-negative id or the diagonal; a row that loses every column keeps the diagonal alone."""
    bs = ids.shape[0]
    eye = torch.eye(bs, dtype=torch.bool)
    same = ((ids[:, None] == ids[None, :]) & (ids[:, None] >= 0)) | eye
    for i in range(bs):
        if bool(same[i].all()):
            same[i] = eye[i]
    return same


def test_sampler_with_distinct_ids_draws_what_the_plain_sampler_draws():
    from alpro_amd.modeling.alpro_models import AlproBaseModel as M
    for bs, seed in ((4, 1), (16, 2), (7, 3)):
        s1, s2 = _sims(bs, seed)
        for ids in (1000 + torch.arange(bs), torch.full((bs,), -1, dtype=I64), torch.full((bs,), 9, dtype=I64)):      # (all equal: the fallback)
            torch.manual_seed(100 + seed)
            want = M._sample_negatives(s1, s2, bs)
            torch.manual_seed(100 + seed)
            got = M._sample_negatives_ids(s1, s2, bs, ids)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (bs, ids)
            assert not s1.requires_grad and got[0].dtype == I64


SAMPLER_IDS = torch.tensor([5, 5, 6, 7, 6, -1, -1, 8, 5, (1 << 40) + 5], dtype=I64)


def test_sampler_never_draws_a_pair_of_the_rows_own_video():
    from alpro_amd.modeling.alpro_models import AlproBaseModel as M
    ids = SAMPLER_IDS
    bs = ids.shape[0]
    s1, s2 = _sims(bs, 11)
    mask = _mask(ids)
    assert int(mask.sum()) == bs + 6 + 2 and not bool(mask[5, 6]) and not bool(mask[0, 9])       # -1 matches no -1; bit 40 counts
    rows = torch.arange(bs)
    for seed in range(200):
        torch.manual_seed(seed)
        nv, nt = M._sample_negatives_ids(s1, s2, bs, ids)
        assert not bool(mask[rows, nv].any()) and not bool(mask[rows, nt].any()), seed


def test_sampler_frequencies_follow_the_masked_softmax():
    """After tests/golden/parity_cases.py::sampler_property_check: every frequency within 4 sigma of the masked softmax weight (fixed seeds,
    so the outcome is one fixed table), and the diagonal-only table of the plain sampler is far off."""
    from alpro_amd.modeling.alpro_models import AlproBaseModel as M
    ids = SAMPLER_IDS
    bs, draws = ids.shape[0], 2000
    s1, s2 = _sims(bs, 12)
    mask = _mask(ids)
    cnt_v, cnt_t = torch.zeros(bs, bs, dtype=I64), torch.zeros(bs, bs, dtype=I64)
    rows = torch.arange(bs)
    torch.manual_seed(77)
    for _ in range(draws):
        nv, nt = M._sample_negatives_ids(s1, s2, bs, ids)
        cnt_v[rows, nv] += 1
        cnt_t[rows, nt] += 1
    for cnt, sim, what in ((cnt_v, s2, "negative video per text"), (cnt_t, s1, "negative text per video")):
        assert int(cnt[mask].sum()) == 0 and int(cnt.sum()) == bs * draws
        pr = torch.softmax(sim.double().masked_fill(mask, -float("inf")), dim=1)
        freq = cnt.double() / draws
        sigma = (pr * (1 - pr) / draws).sqrt()
        z = (freq - pr).abs() / sigma.clamp_min(1e-9)
        z[pr == 0] = 0.0
        assert float(z.max()) < 4.0, "%s: a frequency is %.1f sigma from its masked softmax weight" % (what, float(z.max()))
        plain = sim.double().clone()
        plain.fill_diagonal_(-float("inf"))
        assert float(((freq - torch.softmax(plain, dim=1)).abs() / sigma.clamp_min(1e-9)).max()) > 8.0


# ------------------------------------------------------------------------------------------------ ids for callers
NAMES = ["video7010", "video7010", "video0", "vidéo-ü", "", None, "video7011"]


def _restated(names):
    out = []
    for n in names:
        out.append(-1 if n is None else int.from_bytes(hashlib.blake2b(n.encode("utf-8"), digest_size=8).digest(), "big") & 0x7FFFFFFFFFFFFFFF)
    return out


def test_video_ids_are_a_stable_63_bit_hash():
    from alpro_amd.input_gpu import video_ids
    ids = video_ids(NAMES, device="cpu")
    assert ids.dtype == I64 and ids.shape == (len(NAMES),) and ids.device.type == "cpu"
    assert ids.tolist() == _restated(NAMES)
    assert ids[0] == ids[1] and len(set(ids.tolist())) == len(NAMES) - 1
    assert ids[5] == -1 and all(v >= 0 for i, v in enumerate(ids.tolist()) if i != 5)
    assert video_ids([], device="cpu").shape == (0,)
    code = "from alpro_amd.input_gpu import video_ids; print(video_ids(%r, device='cpu').tolist())" % (NAMES,)
    for seed in ("1", "4242"):
        env = dict(os.environ, PYTHONHASHSEED=seed)
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert eval(r.stdout.strip().splitlines()[-1]) == ids.tolist(), seed


def test_header_and_bindings_declare_the_ids_entry_points():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    for name in ("alpro_vtc_loss_ids_fwd", "alpro_vtc_loss_ids_bwd"):
        assert name in hip.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert hip.ABI_VERSION == 22 and re.search(r"#define\s+ALPRO_HIP_ABI_VERSION\s+22\b", hdr)
    assert callable(hip.vtc_loss_ids_fwd) and callable(hip.vtc_loss_ids_bwd)
    from alpro_amd.modeling import alpro_models as am
    assert issubclass(am._VtcLossIds, torch.autograd.Function)


# ------------------------------------------------------------------------------------------------ the gather of the ids
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from alpro_amd import dist
    dist.init(backend="gloo")
    full = torch.tensor([5, (1 << 62) + 1, -1, 7, 5, (1 << 40) + 5], dtype=I64)
    B = full.shape[0] // world
    ids = full[rank * B:(rank + 1) * B].clone()
    g = dist.allgather(ids)
    assert g.dtype == I64 and torch.equal(g, full) and not g.requires_grad and g.grad_fn is None
    # beside a differentiable gather in one graph: the feature gradient still arrives, nothing is asked of the ids
    v = torch.arange(float(B * 2)).view(B, 2).requires_grad_(True)
    gv = dist.allgather(v)
    assert gv.requires_grad
    (gv * g[:, None].clamp(-1, 9).float()).sum().backward()
    assert v.grad is not None and ids.grad is None
    dist.barrier()
    out.put((rank, "ok"))


def test_world2_gloo_gathers_int64_ids_in_rank_order_without_a_gradient():
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0, "rank process failed (exit %s)" % p.exitcode
    assert sorted(q.get(timeout=5) for _ in range(2)) == [(0, "ok"), (1, "ok")]
