"""GPU: parameter groups in the fused AdamW step (alpro_adamw_step_groups, FlatAdamW with several groups), all through the C ABI -- the
reference's three-group trajectory (tests/golden/optimizer_adamw_groups_4steps.npz), identical groups against the one-group kernel bit for
bit, the kernel against fp64 at ragged sizes and 1 .. the maximum number of segments, loss scaling, no host sync, and two fine-tune steps of
the retrieval model with build_param_groups."""
import math
import os

import numpy as np
import pytest
import torch

from tests import rowwise_cases as rc
from tests.test_hip_ops import _hip

pytestmark = pytest.mark.gpu
TRAJ = dict(rtol=3e-6, atol=2e-8)     # what test_flat_adamw_vs_the_reference_optimizer_trajectory holds the one-group path to
SENTINEL = 12345.0


# ------------------------------------------------------------------------------------------------ 1. reference trajectory
@pytest.mark.parametrize("drive", ["fused", "driver_order"])
def test_flat_adamw_groups_vs_the_reference_optimizer_trajectory(drive):
    _hip()
    import sys
    import alpro_amd.compat
    sys.path.insert(0, alpro_amd.compat.PATH)
    from horovod import torch as hvd
    from alpro_amd import amp, config as rt, optim
    from tests.conftest import GOLDEN
    from tests.golden.groups_init import BASE, STEPS, make_groups
    from tests.test_optim_groups_cpu import _GroupToy
    g = np.load(os.path.join(GOLDEN, "optimizer_adamw_groups_4steps.npz"))
    model = _GroupToy("cuda")
    with rt.use_compute_dtype("fp32"):
        if drive == "fused":
            opt = optim.FlatAdamW(make_groups(list(model.ps)), max_grad_norm=BASE["grad_norm"])
        else:
            opt = hvd.DistributedOptimizer(optim.FlatAdamW(make_groups(list(model.ps))), named_parameters=model.named_parameters(), compression=hvd.Compression.none)
        assert len(opt.param_groups) == 3
        for step in range(STEPS):
            loss = model.loss(step)
            if drive == "fused":
                loss.backward()
                for pg, lr in zip(opt.param_groups, g["lr/%d" % step]):
                    pg["lr"] = float(lr)
                opt.step()
                total = math.sqrt(float(opt.last_grad_norm))
                opt.zero_grad()
            else:
                with amp.scale_loss(loss, opt, delay_unscale=False) as scaled:
                    scaled.backward()
                    optim.zero_none_grad(model)
                    opt.synchronize()
                for pg, lr in zip(opt.param_groups, g["lr/%d" % step]):    # the facade hands out the inner groups
                    pg["lr"] = float(lr)
                views = list(amp.master_params(opt))
                assert len(views) == (len(model.ps) if step == 0 else 1)
                total = float(torch.nn.utils.clip_grad_norm_(views, BASE["grad_norm"]))
                with opt.skip_synchronize():
                    opt.step()
                    opt.zero_grad()
            print("groups trajectory %s step %d: grad norm %r vs %r" % (drive, step, total, float(g["grad_norm/%d" % step])))
            assert total == pytest.approx(float(g["grad_norm/%d" % step]), rel=2e-6)
            got = torch.cat([p.detach().reshape(-1) for p in model.ps]).cpu().numpy().astype(np.float64)
            print("   params max abs err %.3e" % np.abs(got - g["params/%d" % step]).max())
            np.testing.assert_allclose(got, g["params/%d" % step], err_msg="%s step %d" % (drive, step), **TRAJ)
        inner = getattr(opt, "_opt", opt)
        where = {id(p): (o, p.numel()) for p, o in zip(inner.flat["live"], inner.flat["offs"])}
        for key, name in (("m", "exp_avg"), ("v", "exp_avg_sq")):
            flat = torch.cat([inner.flat[key][where[id(p)][0]:sum(where[id(p)])] for p in model.ps]).cpu().numpy()
            np.testing.assert_allclose(flat, g[name], err_msg=name, **TRAJ)
        assert torch.equal(model.frozen.cpu(), torch.ones(11, 3))


# ------------------------------------------------------------------------------------------------ 2. identical groups == one group, bitwise
@pytest.mark.parametrize("split", ["interleaved", "in_layout_order"])
@pytest.mark.parametrize("mode", ["fp16", "bf16"])
def test_identical_groups_are_the_one_group_step_bit_for_bit(mode, split):
    """Three groups with equal hyper-parameters against one group, three steps, p / m / v / the 16-bit mirror compared per parameter (the flat
    layouts differ).  'interleaved': every third tensor per group; the squared norm of a permuted buffer rounds differently, so this split
    runs without the clip.  'in_layout_order': groups that leave the one-group order (matrices, then vectors) as it is -- equal norms, clip on."""
    _hip()
    from alpro_amd import config as rt
    from alpro_amd.optim import FlatAdamW
    shapes = [(64, 48), (48,), (7, 5), (300, 257), (1,), (33, 3, 4), (129,), (1024, 96), (5,)]
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=gen) for s in shapes]
    hp = dict(lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.01, max_grad_norm=0.7 if split == "in_layout_order" else None, allreduce=False)
    with rt.use_compute_dtype(mode):
        a = [torch.nn.Parameter(t.clone().cuda()) for t in init]
        b = [torch.nn.Parameter(t.clone().cuda()) for t in init]
        one = FlatAdamW(a, **hp)
        if split == "interleaved":
            parts = [b[0::3], b[1::3], b[2::3]]
        else:
            mats, vecs = [p for p in b if p.dim() >= 2], [p for p in b if p.dim() < 2]
            parts = [mats[:3], mats[3:] + vecs[:1], vecs[1:]]
        three = FlatAdamW([dict(params=ps) for ps in parts], **hp)
        if mode == "fp16":       # loss scaling: the step size comes from the device counter in both
            for o in (one, three):
                o.scaler.to("cuda").state[0] = 256.0
        for step in range(3):
            grads = [torch.randn(s, generator=gen) * (256.0 if mode == "fp16" else 1.0) for s in shapes]
            for ps, o in ((a, one), (b, three)):
                for p, gr in zip(ps, grads):
                    if o.flat is None:
                        p.grad = gr.clone().cuda()
                    else:
                        p.grad.copy_(gr)
                o._grads_scaled = mode == "fp16"
                o.step()
            off1 = {id(p): o_ for p, o_ in zip(one.flat["live"], one.flat["offs"])}
            off3 = {id(p): o_ for p, o_ in zip(three.flat["live"], three.flat["offs"])}
            same_layout = [off1[id(p)] for p in a] == [off3[id(p)] for p in b]
            assert same_layout == (split == "in_layout_order") and len(three._segments(step + 1)) >= 3
            if same_layout and one.last_grad_norm is not None:
                assert float(one.last_grad_norm) == float(three.last_grad_norm)
            for key in ("p", "m", "v", "lp"):
                for pa, pb in zip(a, b):
                    k = pa.numel()
                    x, y = one.flat[key][off1[id(pa)]:off1[id(pa)] + k], three.flat[key][off3[id(pb)]:off3[id(pb)] + k]
                    assert torch.equal(x, y), "step %d %s of the %s tensor differs" % (step, key, tuple(pa.shape))
            assert float(one.flat["g"].abs().sum()) == 0.0 and float(three.flat["g"].abs().sum()) == 0.0
        assert three.flat["lp"].dtype == {"fp16": torch.float16, "bf16": torch.bfloat16}[mode]
        assert not torch.equal(a[0].detach().cpu(), init[0])


# ------------------------------------------------------------------------------------------------ 3. the kernel against fp64
def make_segments(n, count, seed):
    """`count` segments over [0, n): ends multiples of 4 (the last is n), hyper-parameters different in every segment."""
    gen = rc._gen(900 + seed)
    chunks = (n + 3) // 4
    assert chunks >= count
    if count >= 3 and chunks > 4 * count:      # two one-chunk segments at the front, the other boundaries anywhere (inside waves, mostly)
        cuts = [1, 2] + sorted((torch.randperm(chunks - 3, generator=gen)[:count - 3] + 3).tolist())
    else:
        cuts = sorted((torch.randperm(chunks - 1, generator=gen)[:count - 1] + 1).tolist())
    ends = [c * 4 for c in cuts] + [n]
    segs = []
    for k, e in enumerate(ends):
        lr = 10.0 ** (-2 - (k % 3))
        segs.append(dict(end=e, lr=lr, beta1=(0.9, 0.8, 0.95)[k % 3], beta2=(0.98, 0.999, 0.95)[(k // 2) % 3], eps=(1e-6, 1e-8)[k % 2],
                         weight_decay=(0.01, 0.0, 0.1)[k % 3], step_size=lr * (1.0 + 0.25 * (k % 4)), correct_bias=bool(k % 2)))
    return segs


def groups_ref(ins, segs, **kw):
    outs, start = [], 0
    for s in segs:
        sl = slice(start, s["end"])
        start = s["end"]
        outs.append(rc.adamw_ref(*(t[sl] for t in ins), s["lr"], s["beta1"], s["beta2"], s["eps"], s["weight_decay"], s["step_size"],
                                 correct_bias=s["correct_bias"], **kw))
    return outs


def groups_excess(got, refs, ins, segs):
    worst, start = 0.0, 0
    for s, ref in zip(segs, refs):
        sl = slice(start, s["end"])
        start = s["end"]
        worst = max(worst, rc.adamw_excess([t[sl] for t in got], ref, [t[sl] for t in ins], b1=s["beta1"], b2=s["beta2"]))
    return worst


def run_groups(hip, ins, n, segs, lp_dt=None, **kw):
    bufs = []
    for t in ins:
        buf = torch.full((n + 64,), SENTINEL).cuda()
        buf[:n] = t.cuda()
        bufs.append(buf)
    lp = torch.full((n + 64,), SENTINEL, dtype=lp_dt).cuda() if lp_dt is not None else None
    p, g, m, v = (buf[:n] for buf in bufs)
    hip.adamw_step_groups(p, g, m, v, segs, lp=lp[:n] if lp is not None else None, **kw)
    for buf in bufs + ([lp] if lp is not None else []):
        assert (buf[n:] == SENTINEL).all(), "adamw_step_groups wrote past n=%d" % n
    return p, g, m, v, (lp[:n] if lp is not None else None)


@pytest.mark.parametrize("n", rc.ADAMW_SMALL + rc.ADAMW_BIG)
def test_adamw_step_groups_sizes_segments_and_mirror(n):
    hip = _hip()
    ins = rc.adamw_inputs(n, seed=2)
    norm = (ins[1].double() ** 2).sum().float().reshape(1)
    lp_dt = torch.float16 if n % 2 else torch.bfloat16
    for count in (1, 2, 5, hip.ADAMW_MAX_SEGMENTS):
        if (n + 3) // 4 < count:
            continue
        segs = make_segments(n, count, seed=count)
        assert len(segs) == count
        refs = groups_ref(ins, segs, gnorm_sq=norm, max_norm=2.0)
        p, g, m, v, _ = run_groups(hip, ins, n, segs, gnorm_sq=norm.cuda(), max_norm=2.0)
        assert torch.equal(g.cpu(), ins[1]), "the gradient changed without zero_grad"
        r = groups_excess((p, m, v), refs, ins, segs)
        print("adamw_step_groups n=%d segments=%d: worst error %.3g x the allowance" % (n, count, r))
        assert r <= 1.0, "n=%d, %d segments: worst error is %.3g x the allowance" % (n, count, r)
        p2, g2, m2, v2, lp = run_groups(hip, ins, n, segs, lp_dt=lp_dt, gnorm_sq=norm.cuda(), max_norm=2.0, zero_grad=True)
        assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2), "n=%d: the mirror / zero_grad changed the update" % n
        assert torch.equal(lp, hip.cast(p2.clone(), lp_dt)), "n=%d: mirror != cast of the updated parameters" % n
        assert float(g2.abs().sum()) == 0.0, "zero_grad left gradients behind"


def test_adamw_step_groups_refuses_bad_tables():
    hip = _hip()
    n = 4 * (hip.ADAMW_MAX_SEGMENTS + 8)
    p, g, m, v = (torch.zeros(n).cuda() for _ in range(4))
    seg = dict(lr=1.0, beta1=0.9, beta2=0.9, eps=1e-6, weight_decay=0.0, step_size=1.0, correct_bias=True)
    over = [dict(seg, end=4 * (k + 1)) for k in range(hip.ADAMW_MAX_SEGMENTS)] + [dict(seg, end=n)]
    with pytest.raises(RuntimeError, match="ALPRO_ADAMW_MAX_SEGMENTS = %d" % hip.ADAMW_MAX_SEGMENTS):
        hip.adamw_step_groups(p, g, m, v, over)
    for bad, what in (([dict(seg, end=6), dict(seg, end=n)], "multiples of 4"), ([dict(seg, end=8), dict(seg, end=8), dict(seg, end=n)], "ascend"),
                      ([dict(seg, end=n - 4)], "cover"), ([], "empty")):
        with pytest.raises(RuntimeError, match=what):
            hip.adamw_step_groups(p, g, m, v, bad)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        hip.adamw_step_groups(torch.zeros(n + 1).cuda()[1:], g, m, v, [dict(seg, end=n)])
    assert float(p.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ 4. loss scaling
def test_adamw_step_groups_under_loss_scaling():
    hip = _hip()
    n = 256 * 4 * 3 + 4 * 5 + 3
    segs = make_segments(n, 5, seed=77)
    ins = rc.adamw_inputs(n, seed=3)
    scale, steps = 1024.0, 9.0
    scaled = (ins[0], ins[1] * scale, ins[2], ins[3])
    norm = (scaled[1].double() ** 2).sum().float().reshape(1)
    dyn = (scale, 5.0, steps, 1.0)
    refs = groups_ref(scaled, segs, gnorm_sq=norm, max_norm=2.0, dyn=dyn)     # per segment: bias correction at t = 10 from ITS lr / betas / switch
    dync = torch.tensor(dyn).cuda()
    p, g, m, v, lp = run_groups(hip, scaled, n, segs, lp_dt=torch.float16, gnorm_sq=norm.cuda(), max_norm=2.0, dyn_state=dync)
    r = groups_excess((p, m, v), refs, scaled, segs)
    print("adamw_step_groups loss scaling: worst error %.3g x the allowance" % r)
    assert r <= 1.0 and dync.tolist() == list(dyn)
    assert any(s["correct_bias"] for s in segs) and not all(s["correct_bias"] for s in segs)
    for bad in (float("inf"), float("nan")):       # a non-finite norm: nothing moves in ANY segment, the gradients are consumed
        got = run_groups(hip, scaled, n, segs, lp_dt=torch.float16, gnorm_sq=torch.tensor([bad]).cuda(), max_norm=2.0, dyn_state=dync, zero_grad=True)
        for x, y, what in zip((got[0], got[2], got[3]), (scaled[0], scaled[2], scaled[3]), "pmv"):
            assert torch.equal(x.cpu(), y), "skipped step moved " + what
        assert (got[4] == SENTINEL).all() and float(got[1].abs().sum()) == 0.0
        kept = run_groups(hip, scaled, n, segs, gnorm_sq=torch.tensor([bad]).cuda(), dyn_state=dync, zero_grad=False)
        assert torch.equal(kept[1].cpu(), scaled[1])


def test_flat_adamw_groups_with_the_loss_scaler_skip_and_resume():
    _hip()
    from alpro_amd import config as rt
    from alpro_amd.optim import FlatAdamW
    with rt.use_compute_dtype("fp16"):
        gen = torch.Generator().manual_seed(2)
        ps = [torch.nn.Parameter(torch.randn(s, generator=gen).cuda()) for s in [(64, 48), (48,), (7, 5)]]
        opt = FlatAdamW([dict(params=ps[:2], lr=1e-2), dict(params=ps[2:], lr=1e-3, weight_decay=0.1, correct_bias=False)], allreduce=False)
        sc = opt.scaler.to("cuda")
        for p in ps:
            p.grad = torch.ones_like(p) * 65536.0
        opt._grads_scaled = True
        opt.step()
        before = [p.detach().clone() for p in ps]
        m0, v0, lp0 = opt.flat["m"].clone(), opt.flat["v"].clone(), opt.flat["lp"].clone()
        ps[2].grad[3, 1] = float("inf")
        opt._grads_scaled = True
        opt.step()
        assert all(torch.equal(a, p.detach()) for a, p in zip(before, ps)) and torch.equal(m0, opt.flat["m"]) and torch.equal(v0, opt.flat["v"])
        assert torch.equal(lp0, opt.flat["lp"]) and float(opt.flat["g"].abs().sum()) == 0.0
        assert sc.state.tolist() == [32768.0, 0.0, 1.0, 1.0]
        for p in ps:
            p.grad.fill_(32768.0)
        opt._grads_scaled = True
        opt.step()
        assert sc.state.tolist()[2:] == [2.0, 1.0] and all(not torch.equal(a, p.detach()) for a, p in zip(before, ps))


# ------------------------------------------------------------------------------------------------ 5. no host sync
def test_grouped_step_queues_without_a_host_sync_and_with_the_one_group_launch_count(monkeypatch):
    """torch.cuda.set_sync_debug_mode("error") raises on any synchronising call: a grouped step() -- hyper-parameters rewritten just before, as
    the drivers do -- completes under it, and goes through the library as often as a one-group step: alpro_sumsq, ONE optimizer launch, the
    loss-scale schedule."""
    hip = _hip()
    from alpro_amd import config as rt
    from alpro_amd.optim import FlatAdamW
    log = []
    for name in ("sumsq", "adamw_step", "adamw_step_groups", "loss_scale_update", "cast"):
        def wrap(real, name=name):
            def call(*a, **k):
                log.append(name)
                return real(*a, **k)
            return call
        monkeypatch.setattr(hip, name, wrap(getattr(hip, name)))

    def make(grouped):
        gen = torch.Generator().manual_seed(4)
        ps = [torch.nn.Parameter(torch.randn(s, generator=gen).cuda()) for s in [(64, 48), (48,), (7, 5), (33,)]]
        groups = [dict(params=ps[:2]), dict(params=ps[2:], lr=1e-3, weight_decay=0.1)] if grouped else ps
        return ps, FlatAdamW(groups, lr=1e-2, max_grad_norm=1.0, allreduce=False)

    seen = {}
    with rt.use_compute_dtype("fp16"):
        for grouped in (False, True):
            ps, opt = make(grouped)
            for rep in range(3):
                for p in ps:
                    if opt.flat is None:
                        p.grad = torch.ones_like(p) * 256.0
                    else:
                        p.grad.fill_(256.0)
                opt._grads_scaled = True
                if rep < 2:
                    opt.step()
                    continue
                before = [p.detach().clone() for p in ps]
                torch.cuda.synchronize()
                del log[:]
                torch.cuda.set_sync_debug_mode("error")
                try:
                    for pg in opt.param_groups:          # what a driver does before every step
                        pg["lr"] = pg["lr"] * 0.5
                    opt.step()
                finally:
                    torch.cuda.set_sync_debug_mode("default")
                torch.cuda.synchronize()
                seen[grouped] = list(log)
                assert all(not torch.equal(x, p.detach()) for x, p in zip(before, ps))
    assert seen[False] == ["sumsq", "adamw_step", "loss_scale_update"] and seen[True] == ["sumsq", "adamw_step_groups", "loss_scale_update"]


# ------------------------------------------------------------------------------------------------ 6. model level
def test_two_finetune_steps_of_the_retrieval_model_with_build_param_groups(bert_cfg, monkeypatch):
    _hip()
    from alpro_amd import config as rt
    from alpro_amd.modeling import train as tr
    from alpro_amd.optim import FlatAdamW, build_param_groups
    from tests.golden import parity_cases as pc
    from tests.test_host_cpu import VENC, make_cfg
    from tests.test_model_parity import argmax_multinomial
    m, batch, _ = pc.build_case("retrieval_T2", bert_cfg, VENC, make_cfg, "cuda")
    monkeypatch.setattr(torch, "multinomial", argmax_multinomial)
    base_lr, wd, max_norm = 1e-4, 0.01, 5.0
    groups = build_param_groups(m, lr=base_lr, weight_decay=wd, lr_mult={"visual_encoder.": 0.1})
    assert len(groups) == 4
    opt = FlatAdamW(groups, betas=(0.9, 0.98), max_grad_norm=max_norm, allreduce=False)
    hp_of = {id(p): g for g in opt.param_groups for p in g["params"]}
    name_of = {id(p): n for n, p in m.named_parameters()}
    ref = {}          # id -> [p, m, v] fp64
    worst = 0.0
    with rt.use_compute_dtype("fp32"):
        for step in (1, 2):
            for pg in opt.param_groups:
                pg["lr"] = base_lr * (0.5 if step == 1 else 1.0) * pg["lr_mult"]
            out = m(batch)
            (out["itm_loss"] + out["itc_loss"]).backward()
            trained = [p for p in opt.params if p.grad is not None]
            grads = {id(p): p.grad.detach().double().clone() for p in trained}
            if step == 1:
                ref = {id(p): [p.detach().double().clone(), torch.zeros_like(p, dtype=torch.float64), torch.zeros_like(p, dtype=torch.float64)] for p in trained}
            total = math.sqrt(sum(float((g_ ** 2).sum()) for g_ in grads.values()))
            opt.step()
            assert math.sqrt(float(opt.last_grad_norm)) == pytest.approx(total, rel=2e-6)
            coef = min(max_norm / (total + 1e-6), 1.0)
            for p in trained:      # src/optimization/adamw.py:77-101 per tensor with ITS group's keys, after clip_grad_norm_ over everything
                hp, st = hp_of[id(p)], ref[id(p)]
                b1, b2 = hp["betas"]
                g_ = grads[id(p)] * coef
                st[1] = st[1] * b1 + (1.0 - b1) * g_
                st[2] = st[2] * b2 + (1.0 - b2) * g_ * g_
                step_size = hp["lr"] * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
                st[0] = st[0] - step_size * (st[1] / (st[2].sqrt() + hp["eps"]))
                if hp["weight_decay"] > 0:
                    st[0] = st[0] - hp["lr"] * hp["weight_decay"] * st[0]
                err = float(((p.detach().double() - st[0]).abs() / (TRAJ["atol"] + TRAJ["rtol"] * st[0].abs())).max())
                worst = max(worst, err)
                assert err <= 1.0, "step %d %s: %.3g x the allowance" % (step, name_of[id(p)], err)
            opt.zero_grad()
    print("retrieval fine-tune with 4 groups: worst parameter error %.3g x the trajectory allowance" % worst)
    assert len(opt._segments(2)) <= 8
    layer = m.text_encoder.bert.encoder.layer[0].attention.self
    lins = (layer.query, layer.key, layer.value)
    assert tr.fused_grad_view([l.weight for l in lins]).shape == (3 * 768, 768) and tr.fused_grad_view([l.bias for l in lins]).shape == (3 * 768,)
    assert tr.fused_param_view([l.weight for l in lins]).shape == (3 * 768, 768)
