"""The recomputation switch (alpro_amd.config.recompute_blocks) without a GPU: default, environment variable, context
manager, what Block.slim_saved keeps, and the gradient_checkpointing warning that names the switch."""
import os
import subprocess
import sys
import warnings

import pytest
import torch

from tests.test_host_cpu import VENC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEPT = {"x", "drop_t", "drop_s", "drop_m", "attn_drop", "dims", "dt", "merged", "u_tiled"}


def _child(value):
    env = dict(os.environ)
    env.pop("ALPRO_RECOMPUTE", None)
    if value is not None:
        env["ALPRO_RECOMPUTE"] = value
    return subprocess.run([sys.executable, "-c", "from alpro_amd import config as rt; print('recompute=%d' % rt.recompute_blocks())"],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def test_switch_is_off_by_default_and_follows_the_environment_variable():
    from alpro_amd import config as rt
    if os.environ.get("ALPRO_RECOMPUTE", "0") == "0":
        assert rt.recompute_blocks() is False
    for value, want in ((None, 0), ("0", 0), ("1", 1)):       # a fresh interpreter each: the variable is read once, at load
        r = _child(value)
        assert r.returncode == 0, r.stderr
        assert "recompute=%d" % want in r.stdout, (value, r.stdout)


@pytest.mark.parametrize("value", ["yes", "2", ""])
def test_any_other_value_is_refused_with_a_message(value):
    r = _child(value)
    assert r.returncode != 0
    assert "ALPRO_RECOMPUTE" in r.stderr and "0" in r.stderr and "1" in r.stderr, r.stderr


def test_use_recompute_nests_and_restores_on_exception():
    from alpro_amd import config as rt
    start = rt.recompute_blocks()
    with rt.use_recompute(True):
        assert rt.recompute_blocks() is True
        with rt.use_recompute(False):
            assert rt.recompute_blocks() is False
            with rt.use_recompute(True):
                assert rt.recompute_blocks() is True
            assert rt.recompute_blocks() is False
        assert rt.recompute_blocks() is True
    assert rt.recompute_blocks() is start
    with pytest.raises(KeyError):
        with rt.use_recompute(not start):
            assert rt.recompute_blocks() is (not start)
            raise KeyError("inside")
    assert rt.recompute_blocks() is start


def test_slim_saved_keeps_the_input_the_scales_and_the_scalars_only():
    from alpro_amd.modeling.timesformer.vit import Block
    B, T, N, D, H = 2, 2, 4, 8, 2
    S = 1 + N * T
    t = lambda *shape: torch.randn(*shape)   # noqa: E731
    sv = dict(x=t(B, S, D), dims=(B, T, N, S, D, H), dt=torch.float16, drop_t=t(B * N), drop_s=t(B * T), drop_m=t(B), attn_drop=(0.1, 11, 0.1, 13),
              merged=True, u_tiled=False, h=t(B * N * T, D), qkv_t=t(B * N * T, 3 * D), a_t=t(B * N * T, D), lse_t=t(B * N * H, T), pr=None, xt=t(B, S, D),
              hs=t(B * T * (N + 1), D), qkv_s=t(B * T * (N + 1), 3 * D), a_s=t(B * T * (N + 1), D), lse_s=t(B * T * H, N + 1), x2=t(B, S, D),
              h2=t(B * S, D), u=t(B * S, 4 * D), f1=t(B * S, 4 * D))
    full = dict(sv)
    slim = Block.slim_saved(sv)
    assert set(slim) == KEPT
    tensors = {k for k, v in slim.items() if torch.is_tensor(v)}
    assert tensors == {"x", "drop_t", "drop_s", "drop_m"}
    for k in tensors:
        assert slim[k] is full[k]
    kept_ptrs = {slim[k].data_ptr() for k in tensors}
    assert not [k for k, v in full.items() if torch.is_tensor(v) and k not in tensors and v.data_ptr() in kept_ptrs]
    assert slim["attn_drop"] == (0.1, 11, 0.1, 13) and slim["dims"] == (B, T, N, S, D, H) and slim["dt"] == torch.float16
    assert slim["merged"] is True and slim["u_tiled"] is False
    # a dict of its own: clearing the one it was made from leaves it whole
    sv.clear()
    assert set(slim) == KEPT and all(slim[k] is full[k] for k in KEPT)
    # drop-path off / eval mode: the scale vectors are None and stay None
    none = Block.slim_saved(dict(full, drop_t=None, drop_s=None, drop_m=None))
    assert set(none) == KEPT and {k for k, v in none.items() if torch.is_tensor(v)} == {"x"}


def test_gradient_checkpointing_warning_names_the_switch():
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m = TimeSformer(model_cfg=dict(VENC, num_frm=2, gradient_checkpointing=True), input_format="RGB")
    msgs = [str(x.message) for x in w if "gradient_checkpointing" in str(x.message)]
    assert len(msgs) == 1 and "ignored" in msgs[0] and "ALPRO_RECOMPUTE" in msgs[0] and "use_recompute" in msgs[0], msgs
    assert m.use_grad_ckpt is True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        TimeSformer(model_cfg=dict(VENC, num_frm=2), input_format="RGB")
    assert not [x for x in w if "gradient_checkpointing" in str(x.message) or "ALPRO_RECOMPUTE" in str(x.message)]


def test_the_config_flag_does_not_switch_recomputation_on():
    from alpro_amd import config as rt
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    before = rt.recompute_blocks()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        TimeSformer(model_cfg=dict(VENC, num_frm=2, gradient_checkpointing=True), input_format="RGB")
    assert rt.recompute_blocks() is before
