"""The frozen-prefix decision (alpro_amd.modeling.train.frozen_prefix) and the small helpers that read `requires_grad` for the hand-written
backward, on hand-made stage lists.  No device: the function only looks at the flags."""
import torch

from alpro_amd.modeling import train as tr


def _stage(*flags):
    """One stage = a list of parameters with the given requires_grad flags."""
    return [torch.nn.Parameter(torch.zeros(2), requires_grad=bool(f)) for f in flags]


def test_nothing_frozen():
    assert tr.frozen_prefix([_stage(1, 1), _stage(1, 1), _stage(1)]) == 0


def test_embedding_trainable_blocks_frozen_is_no_prefix():
    assert tr.frozen_prefix([_stage(1, 0), _stage(0, 0), _stage(0, 0)]) == 0


def test_embedding_and_k_blocks_frozen():
    for k in range(4):
        stages = [_stage(0, 0)] + [_stage(0, 0, 0) for _ in range(k)] + [_stage(1, 1, 1) for _ in range(3 - k)]
        assert tr.frozen_prefix(stages) == 1 + k


def test_everything_frozen():
    stages = [_stage(0), _stage(0, 0), _stage(0)]
    assert tr.frozen_prefix(stages) == len(stages)
    assert tr.frozen_prefix([]) == 0


def test_frozen_stage_behind_a_trainable_one_is_not_part_of_the_prefix():
    assert tr.frozen_prefix([_stage(0), _stage(0), _stage(1), _stage(0, 0), _stage(1)]) == 2
    assert tr.frozen_prefix([_stage(1), _stage(0), _stage(0)]) == 0


def test_input_needs_grad_means_no_prefix_whatever_is_frozen():
    assert tr.frozen_prefix([_stage(0), _stage(0), _stage(1)], input_needs_grad=True) == 0
    assert tr.frozen_prefix([_stage(0), _stage(0)], input_needs_grad=True) == 0
    assert tr.frozen_prefix([_stage(0), _stage(0), _stage(1)], input_needs_grad=False) == 2


def test_one_bias_alone_trainable_inside_a_stage_ends_the_prefix():
    assert tr.frozen_prefix([_stage(0, 0), _stage(0, 0, 0, 0), _stage(0, 0, 1, 0), _stage(0, 0)]) == 2


def test_the_flag_is_read_at_every_call():
    stages = [_stage(0), _stage(0), _stage(1)]
    assert tr.frozen_prefix(stages) == 2
    stages[0][0].requires_grad_(True)     # unfrozen later on the same objects
    assert tr.frozen_prefix(stages) == 0
    stages[0][0].requires_grad_(False)
    stages[2][0].requires_grad_(False)
    assert tr.frozen_prefix(stages) == 3


def test_absent_parameters_count_as_frozen():
    assert tr.frozen_prefix([[None], _stage(0) + [None], _stage(1)]) == 2   # (a Linear without bias)


def test_frozen_parameters_get_no_gradient_target():
    p, q = torch.nn.Parameter(torch.zeros(3, 2)), torch.nn.Parameter(torch.zeros(3, 2), requires_grad=False)
    assert tr.trainable(p) and not tr.trainable(q) and not tr.trainable(None)
    assert tr.grad_target(q) is None and q.grad is None and tr.bias_grad(q) is None and tr.bias_grad(None) is None
    g = tr.grad_target(p)
    assert g is p.grad and g.shape == p.shape and float(g.abs().sum()) == 0.0
    tr.add_grad(q, torch.ones(3, 2))
    assert q.grad is None                           # a frozen parameter's .grad stays as it is
    tr.add_grad(p, torch.ones(3, 2))
    tr.add_grad(p, torch.ones(6))
    assert float(p.grad.sum()) == 12.0
    q.requires_grad_(True)                          # ... and the same parameter receives one again once it is unfrozen
    tr.add_grad(q, torch.ones(3, 2))
    assert float(q.grad.sum()) == 6.0
