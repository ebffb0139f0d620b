"""CPU: the host side of TimeSformer.forward_features(pooling='spatial' | 'none') -- the two C entry points (alpro_vit_final_pool_mode and
its backward) are exported and declared under ABI 22, their argument checks answer before anything is launched, the wrappers refuse CPU
tensors, and forward_features keeps the reference's messages (vit.py:475-503) without touching the state dict."""
import ctypes
import json
import os
import re

import pytest
import torch

from tests.conftest import GOLDEN
from tests.test_host_cpu import VENC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("alpro_vit_final_pool_mode", "alpro_vit_final_pool_mode_bwd")


def test_new_entry_points_are_exported_and_declared_under_abi_22():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    lib = hip.load()
    for name in NEW:
        assert name in hip.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, hdr) and hasattr(lib, name), name
    assert "#define ALPRO_HIP_ABI_VERSION 22" in hdr and hip.ABI_VERSION == 22 == lib.alpro_hip_abi_version()
    assert re.search(r"ALPRO_POOL_TEMPORAL = 0, ALPRO_POOL_SPATIAL = 1, ALPRO_POOL_NONE = 2", hdr)
    assert (hip.POOL_TEMPORAL, hip.POOL_SPATIAL, hip.POOL_NONE) == (0, 1, 2)


def test_bad_arguments_are_refused_with_a_message_before_any_launch():
    """mode outside the enum, rows != B * (1 + N * T), D != 768: every check sits in front of the launch, so placeholder addresses are never read."""
    from alpro_amd import hip
    lib = hip.load()
    p = ctypes.c_void_p(4096)
    B, T, N = 2, 3, 9
    rows = B * (1 + N * T)

    def fwd(mode=hip.POOL_SPATIAL, rows=rows, D=768):
        return lib.alpro_vit_final_pool_mode(p, p, p, 1e-6, p, None, hip.F32, mode, rows, B, T, N, D, None)

    def bwd(mode=hip.POOL_SPATIAL, rows=rows, D=768):
        return lib.alpro_vit_final_pool_mode_bwd(p, p, p, 1e-6, p, p, p, mode, rows, B, T, N, D, None, hip.F32, None, 1, None, 0, None)

    for call in (fwd, bwd):
        for kw, msg in ((dict(mode=3), "bad mode 3"), (dict(mode=-1), "bad mode -1"), (dict(rows=rows - 1), "rows=%d is not B" % (rows - 1)),
                        (dict(rows=rows + B), "rows=%d is not B" % (rows + B)), (dict(D=1024), "D=1024 unsupported")):
            assert call(**kw) != 0, kw
            assert msg in lib.alpro_hip_last_error().decode(), (kw, lib.alpro_hip_last_error())


def test_wrappers_refuse_cpu_tensors_and_unknown_modes():
    from alpro_amd import hip
    x, v = torch.zeros(2, 1 + 9 * 3, 768), torch.zeros(768)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.vit_final_pool_mode(x, v, v, 1e-6, 2, 3, 9, torch.float32, hip.POOL_SPATIAL)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.vit_final_pool_mode_bwd(torch.zeros(2, 3, 10, 768), x, v, 1e-6, v.clone(), v.clone(), 2, 3, 9, hip.POOL_NONE)
    with pytest.raises(RuntimeError, match="bad mode"):
        hip.vit_final_pool_mode(x, v, v, 1e-6, 2, 3, 9, torch.float32, 3)


@pytest.fixture(scope="module")
def encoder():
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    return TimeSformer(dict(VENC, num_frm=2), input_format="RGB")


def test_forward_features_keeps_the_reference_messages(encoder):
    x = torch.zeros(1, 3, 2, 224, 224)
    with pytest.raises(AssertionError, match="Invalid pooling type bogus"):
        encoder.forward_features(x, pooling="bogus")
    with pytest.raises(AssertionError, match="Invalid pooling type max"):
        encoder.forward_features(x, return_all_tokens=True, pooling="max")
    with pytest.raises(AssertionError, match="return_all_tokens=False"):
        encoder.forward_features(x, return_all_tokens=False)


@pytest.mark.parametrize("pooling", ["spatial", "none"])
@pytest.mark.parametrize("shape", [(1, 3, 3, 224, 224), (1, 3, 2, 224, 208), (1, 3, 2, 64, 64), (1, 3, 8, 112, 112)])
def test_frame_resolved_modes_refuse_a_geometry_that_is_not_the_configs(encoder, pooling, shape):
    """The reference reshapes by the config's img_size // patch_size and num_frm (vit.py:481-487), so its rearrange raises on any other input; ours
    raises as well, before the device is touched, rather than return differently shaped data.  (8 x 49 tokens = 2 x 196: the same token COUNT as the
    config's, which the reference's rearrange would scramble silently -- refused here too.)"""
    with pytest.raises(RuntimeError, match="the config .* says 2 frames of 14 x 14"):
        encoder.forward_features(torch.zeros(shape), pooling=pooling)


def test_state_dict_keys_are_unchanged(encoder):
    keys = json.load(open(os.path.join(GOLDEN, "state_keys.json")))["retrieval_T2"]
    want = {k[len("visual_encoder."):]: v for k, v in keys.items() if k.startswith("visual_encoder.")}
    assert want and {k: list(v.shape) for k, v in encoder.state_dict().items()} == want
