"""Parameter groups in FlatAdamW, host side (no GPU): constructor rules, the flat layout and segment table, the reference trajectory with
alpro_adamw_step_groups replaced by a restatement of its update, checkpoints, build_param_groups, and the C ABI's new names."""
import ctypes
import json
import math
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# [(parameter index, offset, numel)] and total of tests.test_host_cpu._OptToy under ONE group, recorded from the commit before parameter groups
PARENT_TOY_LAYOUT = [(1, 0, 2368), (3, 2368, 384), (5, 2752, 2368), (7, 5120, 315), (2, 5436, 64), (4, 5500, 1), (6, 5504, 37)]
PARENT_TOY_N = 5544


def P(*shape, grad=True):
    return torch.nn.Parameter(torch.zeros(*shape), requires_grad=grad)


def restated_groups_step(calls, t_of):
    """Stand-in for hip.adamw_step_groups on CPU tensors: the update of the reference's AdamW (src/optimization/adamw.py:77-101) per segment,
    in fp64 rounded once to fp32, with the kernel's scalar plumbing.  Records the segment tables it was given."""
    def fake(p, g, m, v, segments, gnorm_sq=None, max_norm=0.0, grad_scale=1.0, dyn_state=None, grads_scaled=True, zero_grad=False, lp=None):
        assert lp is None and dyn_state is None
        calls.append([dict(s) for s in segments])
        coef = grad_scale
        if gnorm_sq is not None and max_norm > 0:
            coef *= min(max_norm / (math.sqrt(float(gnorm_sq)) * coef + 1e-6), 1.0)
        start = 0
        for s in segments:
            sl = slice(start, s["end"])
            start = s["end"]
            t = t_of()
            step_size = s["lr"] * math.sqrt(1.0 - s["beta2"] ** t) / (1.0 - s["beta1"] ** t) if s["correct_bias"] else s["lr"]
            assert s["step_size"] == pytest.approx(step_size, rel=1e-12)
            gr = g[sl].double() * coef
            mm = m[sl].double() * s["beta1"] + (1.0 - s["beta1"]) * gr
            vv = v[sl].double() * s["beta2"] + (1.0 - s["beta2"]) * gr * gr
            pp = p[sl].double() - step_size * (mm / (vv.sqrt() + s["eps"]))
            if s["weight_decay"] > 0:
                pp = pp - s["lr"] * s["weight_decay"] * pp
            p[sl], m[sl], v[sl] = pp.float(), mm.float(), vv.float()
        if zero_grad:
            g.zero_()
    return fake


def check_segments(opt, segs):
    """<= 2 segments per group, boundaries multiples of 4, covering [0, n); every parameter inside a segment that carries its group's keys."""
    n = opt.flat["n"]
    ends = [s["end"] for s in segs]
    assert ends == sorted(set(ends)) and ends[-1] == n and all(e % 4 == 0 for e in ends)
    assert len(segs) <= 2 * len(opt.param_groups)
    gi = opt._group_index()
    for p, o in zip(opt.flat["live"], opt.flat["offs"]):
        k = next(i for i, e in enumerate(ends) if o < e)
        assert o + p.numel() <= ends[k] and (k == 0 or o >= ends[k - 1])
        grp = opt.param_groups[gi[id(p)]]
        assert (segs[k]["lr"], (segs[k]["beta1"], segs[k]["beta2"]), segs[k]["eps"], segs[k]["weight_decay"], segs[k]["correct_bias"]) == \
               (grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"], grp["correct_bias"])


# ------------------------------------------------------------------------------------------------ constructor
def test_constructor_takes_group_dicts_with_torch_rules():
    from alpro_amd.optim import FlatAdamW
    a, b, c, frozen = P(3, 4), P(5), P(2, 2), P(7, grad=False)
    opt = FlatAdamW([dict(params=[a, frozen], weight_decay=0.0), dict(params=[b, c], lr=5e-4, betas=[0.8, 0.9], eps=1e-8, correct_bias=False)],
                    lr=1e-3, weight_decay=0.05)
    g0, g1 = opt.param_groups
    assert [set(g) for g in (g0, g1)] == [{"params", "lr", "betas", "eps", "weight_decay", "correct_bias"}] * 2
    assert g0["params"] == [a] or (len(g0["params"]) == 1 and g0["params"][0] is a)            # the frozen parameter is dropped from its group
    assert (g0["lr"], g0["betas"], g0["eps"], g0["weight_decay"], g0["correct_bias"]) == (1e-3, (0.9, 0.999), 1e-6, 0.0, True)
    assert (g1["lr"], g1["betas"], g1["eps"], g1["weight_decay"], g1["correct_bias"]) == (5e-4, (0.8, 0.9), 1e-8, 0.05, False)
    assert [id(p) for p in opt.params] == [id(a), id(b), id(c)]
    with pytest.raises(ValueError, match="more than one parameter group"):
        FlatAdamW([dict(params=[a, b]), dict(params=[b])])
    with pytest.raises(ValueError, match="empty"):
        FlatAdamW([])
    one = FlatAdamW(iter([a, frozen, b]), lr=3e-4)                                             # a plain iterable: one group, as ever
    assert len(one.param_groups) == 1 and one.param_groups[0]["params"] is one.params and [id(p) for p in one.params] == [id(a), id(b)]
    assert one.param_groups[0]["lr"] == 3e-4
    single = FlatAdamW([dict(params=a, lr=0.5)])                                               # a bare tensor as 'params', like torch
    assert single.param_groups[0]["params"][0] is a and single.param_groups[0]["lr"] == 0.5


def test_add_param_group_is_refused():
    from alpro_amd.optim import FlatAdamW
    a, b = P(4), P(4)
    opt = FlatAdamW([a], allreduce=False)
    a.grad = torch.ones(4)
    opt._build()
    with pytest.raises(RuntimeError, match="flat buffers are built"):
        opt.add_param_group(dict(params=[b]))


# ------------------------------------------------------------------------------------------------ one group: nothing moves
def test_one_group_layout_and_dispatch_are_the_parent_commits(monkeypatch):
    from alpro_amd import config as rt, hip, optim
    from tests.test_host_cpu import _OptToy
    seen = []
    monkeypatch.setattr(hip, "adamw_step", lambda *a, **k: seen.append("one"))
    monkeypatch.setattr(hip, "adamw_step_groups", lambda *a, **k: seen.append("groups"))
    for params in (lambda m: m.parameters(), lambda m: [dict(params=list(m.parameters()))]):
        model = _OptToy()
        opt = optim.FlatAdamW(params(model), lr=1e-3, allreduce=False)
        model.loss(0).backward()
        with rt.use_compute_dtype("fp32"):
            opt.step()
        assert opt._layout() == PARENT_TOY_LAYOUT and opt.flat["n"] == PARENT_TOY_N
    assert seen == ["one", "one"]


# ------------------------------------------------------------------------------------------------ reference trajectory
class _GroupToy(torch.nn.Module):
    def __init__(self, device="cpu"):
        super().__init__()
        from tests.golden.groups_init import group_tensors
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.clone().to(device)) for _, t in group_tensors("param")])
        self.frozen = torch.nn.Parameter(torch.ones(11, 3, device=device), requires_grad=False)

    def loss(self, step):
        from tests.golden.groups_init import group_tensors
        return sum((p * g.to(p.device)).sum() for p, (_, g) in zip(self.ps, group_tensors("grad", step)))


def test_reference_group_trajectory_through_the_restated_kernel(monkeypatch):
    """Four steps in the drivers' order (lr of the step -> torch's clip over amp.master_params -> step -> zero_grad) on the fixture written by
    tests/golden/make_golden_groups.py from the reference's AdamW with three groups; only the kernel is replaced."""
    from alpro_amd import amp, config as rt, hip, optim
    from tests.conftest import GOLDEN
    from tests.golden.groups_init import BASE, GROUP_HP, STEPS, make_groups
    g = np.load(os.path.join(GOLDEN, "optimizer_adamw_groups_4steps.npz"))
    calls, t = [], [0]
    monkeypatch.setattr(hip, "adamw_step_groups", restated_groups_step(calls, lambda: t[0]))
    monkeypatch.setattr(hip, "adamw_step", lambda *a, **k: pytest.fail("several groups must not take the one-group call"))
    model = _GroupToy()
    groups = make_groups(list(model.ps))
    groups[0]["params"].append(model.frozen)
    with rt.use_compute_dtype("fp32"), mock.patch.object(optim.dist, "collectives_active", lambda: False):
        opt = optim.FlatAdamW(groups)
        assert len(opt.param_groups) == 3 and all(id(p) != id(model.frozen) for p in opt.params)
        for step in range(STEPS):
            t[0] = step + 1
            model.loss(step).backward()
            for pg, lr in zip(opt.param_groups, g["lr/%d" % step]):
                pg["lr"] = float(lr)
            views = list(amp.master_params(opt))
            assert len(views) == (len(model.ps) if step == 0 else 1)          # ONE flat view once the buffers exist, groups or not
            total = float(torch.nn.utils.clip_grad_norm_(views, BASE["grad_norm"]))
            opt.step()
            opt.zero_grad()
            assert total == pytest.approx(float(g["grad_norm/%d" % step]), rel=2e-6)
            check_segments(opt, calls[-1])
            got = torch.cat([p.detach().reshape(-1) for p in model.ps]).numpy()
            np.testing.assert_allclose(got, g["params/%d" % step], rtol=3e-6, atol=2e-8, err_msg="step %d" % step)
        assert len(calls) == STEPS and len(calls[-1]) <= 6
        where = {id(p): (o, p.numel()) for p, o in zip(opt.flat["live"], opt.flat["offs"])}
        for key, name in (("m", "exp_avg"), ("v", "exp_avg_sq")):
            flat = torch.cat([opt.flat[key][where[id(p)][0]:sum(where[id(p)])] for p in model.ps]).numpy()
            np.testing.assert_allclose(flat, g[name], rtol=3e-6, atol=2e-8)
        # order: (group, matrices before vectors, constructor order)
        gi = opt._group_index()
        keys = [(gi[id(p)], p.dim() < 2) for p in opt.flat["live"]]
        assert keys == sorted(keys)
        pos = {id(p): i for i, p in enumerate(opt.params)}
        for k in set(keys):
            idx = [pos[id(p)] for p, kk in zip(opt.flat["live"], keys) if kk == k]
            assert idx == sorted(idx)
        assert [hp["correct_bias"] for hp in GROUP_HP] == [grp["correct_bias"] for grp in opt.param_groups]


def test_hvd_facade_reaches_every_group():
    import sys
    import alpro_amd.compat
    sys.path.insert(0, alpro_amd.compat.PATH)
    from horovod import torch as hvd
    from alpro_amd.optim import FlatAdamW
    inner = FlatAdamW([dict(params=[P(3)], lr=1.0), dict(params=[P(2, 2)], lr=2.0)])
    opt = hvd.DistributedOptimizer(inner)
    for pg in opt.param_groups:
        pg["lr"] = 7.0
    assert [g["lr"] for g in inner.param_groups] == [7.0, 7.0]


def test_fused_qkv_view_follows_the_grouping():
    """q / k / v of a layer in ONE group stay back to back (one fused weight-gradient view); split over groups the view falls back to None."""
    from alpro_amd.modeling import train as tr
    from alpro_amd.optim import FlatAdamW
    for split in (False, True):
        q, k, v, bq, other, wedge = P(8, 8), P(8, 8), P(8, 8), P(8), P(3, 5), P(4, 8)
        groups = [dict(params=[other, q, k] + ([] if split else [v])), dict(params=[bq, wedge] + ([v] if split else []), lr=0.5)]
        opt = FlatAdamW(groups, allreduce=False)
        for p in (q, k, v, bq, other, wedge):
            p.grad = torch.ones_like(p)
        assert opt._build()
        view = tr.fused_grad_view([q, k, v])
        if split:
            assert view is None and tr.fused_param_view([q, k, v]) is None and tr.fused_grad_view([q, k]).shape == (16, 8)
        else:
            assert view.shape == (24, 8) and tr.fused_param_view([q, k, v]).shape == (24, 8)
            view.fill_(2.0)
            assert float(v.grad.sum()) == 128.0 and v.grad.data_ptr() == opt.flat["g"].data_ptr() + 4 * dict(zip(map(id, opt.flat["live"]), opt.flat["offs"]))[id(v)]
        assert set(opt._span) == {id(p) for p in (q, k, v, bq, other, wedge)} and opt._merge(opt._span.values()) == [(0, opt.flat["n"])]


# ------------------------------------------------------------------------------------------------ checkpoints
def _toy_with_groups(monkeypatch, lr_scale=1.0):
    from alpro_amd import hip, optim
    from tests.golden.groups_init import make_groups
    calls = []
    monkeypatch.setattr(hip, "adamw_step_groups", restated_groups_step(calls, lambda: 1))
    model = _GroupToy()
    return model, optim.FlatAdamW(make_groups(list(model.ps), lr=2e-3 * lr_scale), allreduce=False)


def test_state_dict_round_trip_with_groups(monkeypatch):
    from alpro_amd import config as rt
    model, opt = _toy_with_groups(monkeypatch)
    sd0 = opt.state_dict()                                       # before the flat buffers exist
    assert sd0["m"] is None and [sorted(g) for g in sd0["param_groups"]] == [["betas", "correct_bias", "eps", "lr", "params", "weight_decay"]] * 3
    assert sorted(i for g in sd0["param_groups"] for i in g["params"]) == list(range(len(model.ps)))
    model.loss(0).backward()
    with rt.use_compute_dtype("fp32"):
        opt.step()
    sd = json.loads(json.dumps({k: (v.tolist() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}))   # what a saver may do to it
    sd["m"], sd["v"] = torch.tensor(sd["m"]), torch.tensor(sd["v"])
    assert sd["step"] == 1 and len(sd["layout"]) == len(model.ps)

    model2, opt2 = _toy_with_groups(monkeypatch, lr_scale=3.0)
    opt2.load_state_dict(sd)                                      # parked: applied when the first step builds the buffers
    assert opt2.flat is None and opt2.step_count == 1
    assert [g["lr"] for g in opt2.param_groups] == [g["lr"] for g in opt.param_groups] and opt2.param_groups[2]["betas"] == (0.8, 0.95)
    assert opt2.state_dict()["layout"] == [tuple(e) for e in sd["layout"]]
    model2.loss(0).backward()
    opt2._build()
    assert torch.equal(opt2.flat["m"], opt.flat["m"]) and torch.equal(opt2.flat["v"], opt.flat["v"]) and float(opt.flat["v"].abs().sum()) > 0
    opt2.flat["m"].zero_()
    opt2.load_state_dict(sd)                                      # ... and straight into existing buffers
    assert torch.equal(opt2.flat["m"], opt.flat["m"])


def test_parent_format_checkpoint_loads_and_a_grouping_mismatch_raises(monkeypatch):
    from alpro_amd.optim import FlatAdamW
    a, b = P(3, 4), P(5)
    one = FlatAdamW([a, b])
    parent = dict(step=5, param_groups=[dict(lr=3e-4, betas=[0.9, 0.98], eps=1e-6, weight_decay=0.0, correct_bias=True)], layout=[], m=None, v=None)
    one.load_state_dict(parent)
    assert one.step_count == 5 and one.param_groups[0]["lr"] == 3e-4 and one.param_groups[0]["betas"] == (0.9, 0.98)
    assert "params" not in one.state_dict()["param_groups"][0]        # one group keeps writing the format of old
    two = FlatAdamW([dict(params=[a]), dict(params=[b], lr=1.0)])
    with pytest.raises(ValueError, match="grouping .* differs"):
        two.load_state_dict(parent)
    with pytest.raises(ValueError, match="grouping .* differs"):
        one.load_state_dict(two.state_dict())
    c = P(2)
    left, right = FlatAdamW([dict(params=[a, b]), dict(params=[c], lr=1.0)]), FlatAdamW([dict(params=[a]), dict(params=[b, c], lr=2.0)])
    with pytest.raises(ValueError, match="grouping .* differs"):
        right.load_state_dict(dict(left.state_dict(), step=9))
    assert right.param_groups[1]["lr"] == 2.0 and right.step_count == 0 and one.param_groups[0]["lr"] == 3e-4     # a refused checkpoint changed nothing


# ------------------------------------------------------------------------------------------------ build_param_groups
def test_build_param_groups_on_the_retrieval_models_names():
    from alpro_amd.optim import FlatAdamW, build_param_groups
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "state_keys.json")))["retrieval_T2"]
    names = [n for n in keys if not n.endswith("position_ids")]
    named = [(n, P(1)) for n in names]
    name_of = {id(p): n for n, p in named}
    groups = build_param_groups(named, lr=1e-4, weight_decay=0.01, lr_mult={"visual_encoder.": 0.1, "text_encoder.": 0.1})
    by = {(g["weight_decay"] > 0, g["lr_mult"]): {name_of[id(p)] for p in g["params"]} for g in groups}
    assert set(by) == {(True, 1.0), (False, 1.0), (True, 0.1), (False, 0.1)} and sum(len(s) for s in by.values()) == len(names)
    assert by[(True, 1.0)] == {"itm_head.weight", "text_proj.weight", "vision_proj.weight", "temp"}
    assert by[(False, 1.0)] == {"itm_head.bias", "text_proj.bias", "vision_proj.bias"}
    for n in names:
        if n.startswith(("visual_encoder.", "text_encoder.")):
            no_decay = n.endswith(".bias") or "LayerNorm" in n or "norm" in n or ".embeddings." in n
            assert n in by[(not no_decay, 0.1)], n
    assert "visual_encoder.model.blocks.3.attn.qkv.weight" in by[(True, 0.1)] and "visual_encoder.model.blocks.3.temporal_norm1.weight" in by[(False, 0.1)]
    assert "text_encoder.bert.embeddings.word_embeddings.weight" in by[(False, 0.1)]
    for g in groups:
        assert g["lr"] == pytest.approx(1e-4 * g["lr_mult"]) and g["weight_decay"] in (0.0, 0.01)
    # q / k / v of one BERT layer share a group, so they stay neighbours in the flat layout
    qkv = ["text_encoder.bert.encoder.layer.0.attention.self.%s.weight" % k for k in ("query", "key", "value")]
    assert all(n in by[(True, 0.1)] for n in qkv)
    opt = FlatAdamW(groups)
    assert len(opt.param_groups) == 4 and opt.param_groups[0]["lr_mult"] in (1.0, 0.1)


def test_build_param_groups_honours_no_weight_decay_of_submodules():
    from alpro_amd.optim import build_param_groups

    class Enc(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.pos_embed, self.proj, self.off = P(1, 4, 8), torch.nn.Linear(8, 8), P(3, grad=False)

        def no_weight_decay(self):
            return {"pos_embed"}

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.visual, self.head = Enc(), torch.nn.Linear(8, 2)
            self.tied = self.head.weight

    net = Net()
    groups = build_param_groups(net, lr=1.0, weight_decay=0.1, lr_mult={"visual.": 0.5, "visual.proj.": 0.25})
    got = {(g["weight_decay"], g["lr_mult"]): {id(p) for p in g["params"]} for g in groups}
    assert got == {(0.0, 0.5): {id(net.visual.pos_embed)}, (0.1, 0.25): {id(net.visual.proj.weight)}, (0.0, 0.25): {id(net.visual.proj.bias)},
                   (0.1, 1.0): {id(net.head.weight)}, (0.0, 1.0): {id(net.head.bias)}}
    assert sum(len(g["params"]) for g in groups) == 5


# ------------------------------------------------------------------------------------------------ C ABI
def test_library_and_header_carry_the_grouped_step():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    assert re.search(r"\bint\s+alpro_adamw_step_groups\s*\(", hdr) and "alpro_adamw_step_groups" in hip.EXPORTS
    bound = int(re.search(r"#define ALPRO_ADAMW_MAX_SEGMENTS (\d+)", hdr).group(1))
    assert bound >= 16 and bound == hip.ADAMW_MAX_SEGMENTS
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), "alpro_adamw_step_groups")
    fields = re.search(r"typedef struct alpro_adamw_segment_t \{(.*?)\}", hdr, re.S).group(1)
    names = [n for decl in re.findall(r"(?:int64_t|int32_t|float)\s+([^;]+);", fields) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [f[0] for f in hip.AdamWSegment._fields_] and ctypes.sizeof(hip.AdamWSegment) == 40
    assert ctypes.sizeof(hip.AdamWSegments) == 8 + 40 * bound
    assert hip.ABI_VERSION == 22
    with pytest.raises(RuntimeError, match="device tensors"):
        z = torch.zeros(8)
        hip.adamw_step_groups(z, z, z, z, [dict(end=8, lr=1.0, beta1=0.9, beta2=0.9, eps=1e-6, weight_decay=0.0, step_size=1.0, correct_bias=True)])
