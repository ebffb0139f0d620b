"""`src.optimization.adamw.AdamW` (reference adamw.py:12-103) -> alpro_amd.optim.FlatAdamW: same constructor arguments and defaults
(a parameter list or torch-style group dicts with their own lr / betas / eps / weight_decay / correct_bias; lr 1e-3, betas (0.9, 0.999),
eps 1e-6, weight_decay 0.0, correct_bias True), same update (pinned by tests/golden/optimizer_adamw_3steps.npz and, with three groups,
optimizer_adamw_groups_4steps.npz), as two launches over flat buffers instead of ~930 per-tensor Python iterations.  Not a
torch.optim.Optimizer subclass: no add_param_group, no torch LR schedulers."""
from alpro_amd.optim import FlatAdamW as AdamW  # noqa: F401
