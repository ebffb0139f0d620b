"""CPU: the host side of the visual encoder's attention-gradient / Grad-CAM output -- alpro_attn_temporal_probs_grad's ABI surface and argument
checks (every check sits in front of the first HIP call, so placeholder addresses are never read), the self-check of the case builders
(tests/attn_temporal_probs_grad_cases.py), and the refusals of the wrapper, of VitAttnGradients, of forward_features(attn_grads=) and of the two
grounding helpers that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import attn_probs_grad_cases as gc
from tests import attn_temporal_probs_grad_cases as tg
from tests.test_host_cpu import VENC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_point_is_exported_and_declared_and_the_abi_number_stays():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    lib = hip.load()
    name = "alpro_attn_temporal_probs_grad"
    assert name in hip.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, hdr) and hasattr(lib, name)
    assert "#define ALPRO_HIP_ABI_VERSION 22" in hdr and hip.ABI_VERSION == 22 == lib.alpro_hip_abi_version()   # additive: one new symbol
    assert os.path.exists(os.path.join(ROOT, "alpro_amd", "csrc", "attention_temporal_probs_grad.hip"))
    assert callable(hip.attn_temporal_probs_grad)


def test_bad_arguments_are_refused_with_a_message_and_without_a_device():
    from alpro_amd import hip
    lib = hip.load()
    p = ctypes.c_void_p(4096)
    good = dict(qkv=p, dctx=p, lse=p, grad=p, cam=p, dtype=hip.F16, rows=40, T=8, H=2)

    def call(**kw):
        a = dict(good, **kw)
        return lib.alpro_attn_temporal_probs_grad(a["qkv"], a["dctx"], a["lse"], a["grad"], a["cam"], a["dtype"], a["rows"], a["T"], a["H"], 0.125, 1.0, None)

    for kw, msg in ((dict(dtype=3), "dtype=3"), (dict(dtype=-1), "dtype=-1"),
                    (dict(T=0), "num_frm=0"), (dict(T=129, rows=129), "num_frm=129"), (dict(T=-8), "num_frm=-8"),
                    (dict(T=3), "rows=40 not a non-negative multiple of T=3"), (dict(rows=-8), "rows=-8"),
                    (dict(H=0), "H=0"),
                    (dict(grad=None, cam=None), "null grad_out and null cam_out"),
                    (dict(qkv=None), "null qkv"), (dict(dctx=None), "null dctx"), (dict(lse=None), "null lse"),
                    (dict(qkv=ctypes.c_void_p(4096 + 8)), "16-byte aligned"), (dict(dctx=ctypes.c_void_p(4096 + 2)), "16-byte aligned"),
                    (dict(grad=ctypes.c_void_p(4096 + 4)), "16-byte aligned"), (dict(cam=ctypes.c_void_p(4096 + 4), grad=None), "16-byte aligned"),
                    (dict(lse=ctypes.c_void_p(4096 + 2)), "4-byte aligned")):
        rc = call(**kw)
        assert rc != 0, kw
        err = lib.alpro_hip_last_error().decode()
        assert msg in err and "alpro_attn_temporal_probs_grad" in err, (kw, err)
    # rows == 0 is a no-op that reads no pointer (rows % 32 need not be 0: 40 above is fine as far as the checks go)
    assert call(rows=0, qkv=None, dctx=None, lse=None, grad=None, cam=None) == 0


def test_the_forward_entry_point_keeps_its_refusals():
    """alpro_attn_temporal_probs shares its shape checks with the new entry point (attn_map.hpp): same words, its own name."""
    from alpro_amd import hip
    lib = hip.load()
    p = ctypes.c_void_p(4096)
    for args, msg in (((p, p, p, hip.F16, 40, 3, 2), "alpro_attn_temporal_probs: rows=40 not a non-negative multiple of T=3"),
                      ((p, p, p, hip.F16, 40, 0, 2), "alpro_attn_temporal_probs: num_frm=0 unsupported"),
                      ((p, p, p, 7, 40, 8, 2), "alpro_attn_temporal_probs: dtype=7"),
                      ((p, p, p, hip.F16, 40, 8, 0), "alpro_attn_temporal_probs: H=0"),
                      ((p, p, None, hip.F16, 40, 8, 2), "alpro_attn_temporal_probs: null out")):
        assert lib.alpro_attn_temporal_probs(*args, 0.125, None) != 0
        assert msg in lib.alpro_hip_last_error().decode(), (msg, lib.alpro_hip_last_error())


def test_wrapper_refuses_cpu_tensors_and_a_bad_want():
    from alpro_amd import hip
    qkv, dctx, lse = torch.zeros(16, 3 * 2 * 64), torch.zeros(16, 2 * 64), torch.zeros(1, 2, 32)
    with pytest.raises(RuntimeError, match="attn_temporal_probs_grad: qkv must be a device tensor.*no CPU fallback"):
        hip.attn_temporal_probs_grad(qkv, dctx, lse, 8, 2, 0.125)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attn_temporal_probs_grad(np.zeros((16, 384), dtype=np.float32), dctx, lse, 8, 2, 0.125)
    for want in ((), ("probs",), ("cam", "cam"), "map"):
        with pytest.raises(RuntimeError, match="want="):
            hip.attn_temporal_probs_grad(qkv, dctx, lse, 8, 2, 0.125, want=want)


@pytest.mark.parametrize("dtype", tg.DTYPES)
def test_case_builders_hold_what_they_claim(dtype):
    T, groups, H = 5, 3, 2
    for small in (False, True):
        g = tg.temporal_grad_case(T, dtype, groups, H=H, small=small)
        c = g.case
        assert (c.batch, c.L, c.H, c.bias) == (groups, T, H, None)
        assert g.dctx.shape == (groups * T, H * 64) and g.grad_scale == (1024.0 if small else 1.0)
        qkv = c.qkv.astype(np.float64)
        for grp, h, q, k in ((0, 0, 0, 0), (2, 1, 4, 2), (1, 1, 3, 4), (2, 0, 2, 2)):   # G64 of group grp = rows grp*T .. grp*T + T - 1, a plain loop
            want = 0.0
            for i in range(64):
                want += float(g.dctx[grp * T + q, h * 64 + i]) * float(qkv[grp * T + k, 2 * H * 64 + h * 64 + i])
            assert abs(g.g64[grp, h, q, k] - g.grad_scale * want) <= 1e-12 * max(1.0, abs(want) * g.grad_scale)
        assert np.array_equal(g.cam64, c.p64 * np.maximum(g.g64, 0.0)) and (g.g64 < 0).any() and (g.g64 > 0).any()
        assert np.abs(c.p64.sum(-1) - 1.0).max() < 1e-12
    pk = tg.temporal_grad_case(8, dtype, 2, H=H, peaked=True)
    assert np.abs(pk.case.s64).max() > 30.0      # the peaked regime of attn_probs_cases


def test_the_softmax_backward_from_the_maps_is_autograd_s():
    """dqkv_from_maps (the cross-check against alpro_attn_temporal_bwd) against torch autograd in fp64 on the case's own numbers."""
    g = tg.temporal_grad_case(5, "fp32", 3, H=2)
    c = g.case
    x = torch.from_numpy(c.qkv.astype(np.float64)).requires_grad_(True)
    t = x.view(c.batch, c.L, 3, c.H, 64).permute(2, 0, 3, 1, 4)
    p = ((t[0] @ t[1].transpose(-1, -2)) * c.scale).softmax(-1)
    out = (p @ t[2]).transpose(1, 2).reshape(c.batch * c.L, c.H * 64)
    out.backward(torch.from_numpy(g.dctx.astype(np.float64)))
    assert np.abs(p.detach().numpy() - c.p64).max() < 1e-14
    got = tg.dqkv_from_maps(c, g.dctx, c.p64, g.g64)
    assert got.shape == tuple(x.grad.shape) and np.abs(got - x.grad.numpy()).max() <= 1e-12 * np.abs(x.grad.numpy()).max()


def test_collector_validates_its_arguments_and_refuses_an_early_read():
    from alpro_amd.modeling.timesformer.vit import VitAttnGradients
    with pytest.raises(ValueError, match="want="):
        VitAttnGradients(want=("probs",))
    with pytest.raises(ValueError, match="no layer chosen"):
        VitAttnGradients(layers=())
    with pytest.raises(ValueError, match="grad_scale"):
        VitAttnGradients(grad_scale=0.0)
    with pytest.raises(ValueError, match="nothing to collect"):
        VitAttnGradients(spatial=False, temporal=False)
    with pytest.raises(ValueError, match="spatial_window must be"):
        VitAttnGradients(spatial_window=(0, 1))
    col = VitAttnGradients(layers=(-1, 0), want=("grad", "cam"))
    for name in ("spatial_grads", "spatial_cams", "temporal_grads", "temporal_cams"):
        with pytest.raises(RuntimeError, match="not passed to"):
            getattr(col, name)
    with pytest.raises(ValueError, match="block index 12 outside"):
        VitAttnGradients(layers=(12,)).begin(12)
    col.begin(12)
    assert col.wants(0) and col.wants(11) and not col.wants(5) and col.first() == 0
    with pytest.raises(RuntimeError, match=r"backward\(\) has not run through block 0 \(spatial\), block 0 \(temporal\), block 11"):
        col.temporal_cams
    only = VitAttnGradients(want="cam", temporal=False)
    only.begin(2)
    assert only._pending == {("spatial", 0), ("spatial", 1)}
    only._pending.clear()
    with pytest.raises(RuntimeError, match="want="):
        only.spatial_grads
    with pytest.raises(RuntimeError, match="temporal=False"):
        only.temporal_cams
    assert only.spatial_cams == {}


def _encoder(**kw):
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    return TimeSformer(model_cfg=dict(VENC, num_frm=2, img_size=32, **kw), input_format="RGB")


def test_forward_features_refuses_no_grad_active_attention_dropout_and_forward_cls_without_a_device():
    from alpro_amd.modeling.timesformer.vit import VitAttnGradients
    x = torch.zeros(1, 3, 2, 32, 32)
    enc = _encoder().eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="grad mode is off"):
        enc.forward_features(x, attn_grads=VitAttnGradients())
    with pytest.raises(TypeError, match="VitAttnGradients"):
        enc.forward_features(x, attn_grads=object())
    with pytest.raises(ValueError, match="block index 12 outside"):
        enc.forward_features(x, attn_grads=VitAttnGradients(layers=(12,)))
    with torch.no_grad(), pytest.raises(TypeError, match="forward_cls takes no attn_grads"):
        enc.forward_cls(x, attn_grads=VitAttnGradients())
    drop = _encoder(attn_drop_rate=0.1).train()
    with pytest.raises(RuntimeError, match=r"block 3 has active attention dropout.*model\.eval\(\)"):
        drop.forward_features(x, attn_grads=VitAttnGradients(layers=(3, -1)))


@pytest.mark.parametrize("name", ("frame_patch_gradcam", "patch_temporal_gradcam"))
def test_helpers_refuse_train_mode_a_ragged_clip_mismatched_captions_and_a_scale_that_is_no_power_of_two(name):
    from alpro_amd import grounding
    fn = getattr(grounding, name)
    m = torch.nn.Module().train()
    ids = torch.zeros(2, 8, dtype=torch.long)
    clip = torch.zeros(2, 2, 3, 32, 32)
    with pytest.raises(RuntimeError, match=r"%s.*model\.eval\(\)" % name):
        fn(m, ids, torch.ones_like(ids), clip)
    m.eval()
    with pytest.raises(ValueError, match="multiples of the 16-pixel patch"):
        fn(m, ids, torch.ones_like(ids), torch.zeros(2, 2, 3, 32, 40))
    with pytest.raises(ValueError, match="one caption per clip"):
        fn(m, ids[:1], torch.ones_like(ids[:1]), clip)
    with pytest.raises(ValueError, match="power of two"):
        fn(m, ids, torch.ones_like(ids), clip, grad_scale=3.0)
