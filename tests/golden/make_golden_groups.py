"""Writes tests/golden/optimizer_adamw_groups_4steps.npz: the REFERENCE's AdamW (src/optimization/adamw.py) with three parameter groups that
differ in every key, its get_lr_sched (src/optimization/sched.py) and torch's clip_grad_norm_, driven for four steps in the order of the
reference's drivers (lr of the step -> clip -> step -> zero_grad) on the closed-form tensors of tests/golden/groups_init.py.

    python -m tests.golden.make_golden_groups        (authoring container only: needs the reference checkout, see ref_harness.py)
"""
import os
import warnings

import numpy as np
import torch

from tests.golden import ref_harness as rh
from tests.golden.groups_init import BASE, GROUP_HP, STEPS, group_tensors, make_groups

HERE = os.path.dirname(os.path.abspath(__file__))


def case_optimizer_groups(fname):
    from torch.nn.utils import clip_grad_norm_
    from src.optimization.adamw import AdamW
    from src.optimization.sched import get_lr_sched
    params = [torch.nn.Parameter(t.clone()) for _, t in group_tensors("param")]
    opt = AdamW(make_groups(params))
    g = {}
    for step in range(STEPS):
        for p_, (_, gr) in zip(params, group_tensors("grad", step)):
            p_.grad = gr.clone()
        lr_this_step = get_lr_sched(step + 1, BASE["decay"], BASE["lr"], BASE["num_train_steps"], warmup_ratio=BASE["warmup_ratio"])
        for pg, hp in zip(opt.param_groups, GROUP_HP):
            pg["lr"] = lr_this_step * hp["lr_mult"]
        total = clip_grad_norm_(params, BASE["grad_norm"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")     # the deprecated add_(Number, Tensor) overloads of the reference still run on this torch
            opt.step()
        opt.zero_grad()
        g["lr/%d" % step] = np.array([pg["lr"] for pg in opt.param_groups], dtype=np.float64)
        g["grad_norm/%d" % step] = np.float64(float(total))
        g["params/%d" % step] = np.concatenate([p_.detach().numpy().astype(np.float32).reshape(-1) for p_ in params])
    g["exp_avg"] = np.concatenate([opt.state[p_]["exp_avg"].numpy().reshape(-1) for p_ in params])
    g["exp_avg_sq"] = np.concatenate([opt.state[p_]["exp_avg_sq"].numpy().reshape(-1) for p_ in params])
    np.savez_compressed(os.path.join(HERE, fname), **g)


if __name__ == "__main__":
    rh.import_reference()
    torch.set_num_threads(8)
    case_optimizer_groups("optimizer_adamw_groups_4steps.npz")
