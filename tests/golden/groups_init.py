"""Closed-form inputs of the parameter-group optimizer fixture (tests/golden/optimizer_adamw_groups_4steps.npz): a dozen tensors with 2-D and
1-D shapes interleaved in constructor order and sizes that are not multiples of 4, split over three groups that differ in every
hyper-parameter.  Shared by make_golden_groups.py (which drives the reference's AdamW on them) and the tests; TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

from tests.golden.det_init import unit_uniform

STEPS = 4
# (name, shape, group): constructor order is this order
GROUP_TENSORS = [
    ("enc.w0", (37, 13), 1), ("enc.b0", (37,), 0), ("head.w", (5, 9), 2), ("enc.w1", (64, 48), 1), ("enc.ln.weight", (48,), 0),
    ("enc.ln.bias", (48,), 0), ("head.b", (5,), 2), ("enc.w2", (21, 7), 1), ("emb.table", (101, 6), 0), ("enc.b1", (1,), 0),
    ("head.w2", (3, 3, 2), 2), ("enc.w3", (130, 33), 1), ("head.scale", (), 2),
]
BASE = dict(lr=2e-3, decay="linear", num_train_steps=10, warmup_ratio=0.2, grad_norm=1.5)
# per group: lr multiplier and every other key different; group 2 without bias correction
GROUP_HP = [
    dict(lr_mult=1.0, weight_decay=0.0, betas=(0.9, 0.98), eps=1e-6, correct_bias=True),
    dict(lr_mult=0.1, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8, correct_bias=True),
    dict(lr_mult=2.0, weight_decay=0.1, betas=(0.8, 0.95), eps=1e-6, correct_bias=False),
]
GRAD_SCALES = (1.0, 0.03, 4.0, 0.5)   # step 2 is clipped hard, step 1 not at all


def group_tensors(kind, step=0):
    """[(name, tensor)] in constructor order: kind 'param', or 'grad' of `step`."""
    out = []
    for name, shape, _ in GROUP_TENSORS:
        n = int(np.prod(shape)) if len(shape) else 1
        if kind == "param":
            v = 0.05 * unit_uniform("groups/param/" + name, n)
        else:
            v = GRAD_SCALES[step] * 0.1 * unit_uniform("groups/grad/%d/%s" % (step, name), n)
        out.append((name, torch.from_numpy(np.asarray(v, dtype=np.float32).reshape(shape))))
    return out


def make_groups(params, lr=None):
    """The three group dicts over `params` (constructor order), at learning rate `lr` x multiplier (default: the base rate)."""
    lr = BASE["lr"] if lr is None else lr
    groups = []
    for k, hp in enumerate(GROUP_HP):
        groups.append(dict(params=[p for p, (_, _, g) in zip(params, GROUP_TENSORS) if g == k], lr=lr * hp["lr_mult"], betas=hp["betas"], eps=hp["eps"],
                           weight_decay=hp["weight_decay"], correct_bias=hp["correct_bias"]))
    return groups
