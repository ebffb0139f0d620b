"""CPU: the host side of the visual encoder's attention-map output -- alpro_attn_temporal_probs' ABI surface and argument checks (every check sits
in front of the first HIP call, so placeholder addresses are never read), the lse re-layout helpers of tests/attn_temporal_probs_cases.py, and the
refusals of the wrapper, of the collector's arguments, of forward_cls and of the two grounding helpers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import attn_temporal_probs_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_point_is_exported_and_declared_under_abi_22():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    lib = hip.load()
    assert "alpro_attn_temporal_probs" in hip.EXPORTS and re.search(r"\bint\s+alpro_attn_temporal_probs\s*\(", hdr) and hasattr(lib, "alpro_attn_temporal_probs")
    assert "#define ALPRO_HIP_ABI_VERSION 22" in hdr and hip.ABI_VERSION == 22 == lib.alpro_hip_abi_version()
    assert "#define ALPRO_ATTN_MAX_T 128" in hdr
    assert "vit.py:92-93" in hdr and "vit.py:147" in hdr


def test_bad_arguments_are_refused_with_a_message_that_names_the_value():
    from alpro_amd import hip
    lib = hip.load()
    p = ctypes.c_void_p(4096)
    good = dict(qkv=p, lse=p, out=p, dtype=hip.F16, rows=40, T=8, H=2)

    def call(**kw):
        a = dict(good, **kw)
        return lib.alpro_attn_temporal_probs(a["qkv"], a["lse"], a["out"], a["dtype"], a["rows"], a["T"], a["H"], 0.125, None)

    for kw, msg in ((dict(T=0), "num_frm=0 unsupported (1..128 = ALPRO_ATTN_MAX_T)"), (dict(T=129, rows=129), "num_frm=129 unsupported (1..128 = ALPRO_ATTN_MAX_T)"),
                    (dict(T=-8), "num_frm=-8"), (dict(rows=41), "rows=41 not a non-negative multiple of T=8"), (dict(rows=-8), "rows=-8"),
                    (dict(T=3, rows=40), "rows=40 not a non-negative multiple of T=3"), (dict(dtype=3), "dtype=3"), (dict(dtype=-1), "dtype=-1"),
                    (dict(H=0), "H=0"), (dict(H=-2), "H=-2"), (dict(qkv=None), "null qkv"), (dict(lse=None), "null lse"), (dict(out=None), "null out"),
                    (dict(out=ctypes.c_void_p(4096 + 4)), "16-byte aligned"), (dict(qkv=ctypes.c_void_p(4096 + 8)), "16-byte aligned"),
                    (dict(lse=ctypes.c_void_p(4096 + 2)), "lse must be 4-byte aligned")):
        rc = call(**kw)
        assert rc != 0, kw
        assert msg in lib.alpro_hip_last_error().decode(), (kw, lib.alpro_hip_last_error())
    # no rows: a no-op success, whatever the pointers are -- but still only for arguments that make sense
    assert call(rows=0) == 0 and call(rows=0, qkv=None, lse=None, out=None) == 0
    assert call(rows=0, T=0) != 0 and call(rows=0, dtype=7) != 0


def test_wrapper_refuses_cpu_tensors():
    from alpro_amd import hip
    qkv, lse = torch.zeros(16, 3 * 2 * 64), torch.zeros(1, 2, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attn_temporal_probs(qkv, lse, 8, 2, 0.125)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attn_temporal_probs(np.zeros((16, 384), dtype=np.float32), lse, 8, 2, 0.125)


@pytest.mark.parametrize("groups,T,H", [(1, 1, 1), (5, 3, 2), (37, 7, 2), (4, 8, 3), (3, 33, 2), (2, 128, 1), (1, 32, 2)])
def test_lse_relayout_against_a_loop(groups, T, H):
    rng = np.random.RandomState(groups * 1000 + T)
    lse = rng.standard_normal((groups, H, T)).astype(np.float32)
    ch = tc.lse_to_chunks(lse, fill=-7.0)
    rows = groups * T
    assert ch.shape == ((rows + 31) // 32, H, 32) and ch.flags["C_CONTIGUOUS"] and ch.dtype == np.float32
    seen = np.zeros(ch.shape, dtype=bool)
    for g in range(groups):
        for h in range(H):
            for t in range(T):
                row = g * T + t
                assert ch[row // 32, h, row % 32] == lse[g, h, t]
                seen[row // 32, h, row % 32] = True
    assert (ch[~seen] == -7.0).all() and (~seen).sum() == (ch.shape[0] * 32 - rows) * H
    assert np.array_equal(tc.lse_from_chunks(ch, groups, T), lse)


def test_temporal_cases_are_the_spatial_cases_with_batch_groups():
    c = tc.temporal_case(5, "fp16", 37)
    assert (c.batch, c.L, c.H) == (37, 5, 2) and c.bias is None and c.qkv.shape == (37 * 5, 3 * 2 * 64)
    assert c.p64.shape == (37, 2, 5, 5) and np.abs(c.p64.sum(-1) - 1.0).max() < 1e-12
    d = tc.case_from_qkv("again", c.qkv, 37, 5, 2, "fp16")
    assert np.array_equal(d.p64, c.p64) and np.array_equal(d.lse64, c.lse64)
    pk = tc.peaked_temporal_case(33, "fp32", 5)
    assert pk.p64.shape == (5, 2, 33, 33) and 55.0 < np.abs(pk.s64).max() < 70.0
    assert all(g * T % 32 != 0 for g in tc.GROUPS for T in tc.FRAMES if T not in (32, 64, 128))


def test_collector_arguments():
    from alpro_amd.modeling.timesformer import vit
    assert vit._collector(12, False, False, None, None) is None                 # flags off: no collector object at all
    c = vit._collector(12, True, False, (-1, 0, 11), ((0, 1), (1, 10)))
    assert c.layers == {0, 11} and c.q_range == (0, 1) and c.k_range == (1, 10) and c.want_attn and not c.want_hidden
    assert [bool(c.block_begin()) for c.i in range(12)] == [True] + [False] * 10 + [True]
    h = vit._collector(12, False, True, None, None)
    assert h.layers == set(range(12)) and h.block_begin() is None               # hidden states only: no block collects maps
    r = h.result("f")
    assert r.features == "f" and r.hidden_states == () and r.spatial_attentions is None and r.temporal_attentions is None
    with pytest.raises(ValueError, match="attn_layers: block index 12"):
        vit._collector(12, True, False, (12,), None)
    with pytest.raises(ValueError, match="attn_layers: block index -13"):
        vit._collector(12, True, False, (-13,), None)
    with pytest.raises(ValueError, match="attn_window must be"):
        vit._collector(12, True, False, None, (0, 1))


def test_forward_cls_takes_no_flags():
    from alpro_amd.modeling.timesformer.vit import TimeSformer
    with pytest.raises(TypeError, match="forward_cls takes no output_attentions"):
        TimeSformer.forward_cls(None, torch.zeros(1), output_attentions=True)


def test_helpers_refuse_train_mode_and_bad_arguments():
    from alpro_amd.grounding import frame_patch_attention, patch_temporal_attention
    enc = torch.nn.Module().train()
    holder = torch.nn.Module()
    holder.visual_encoder = enc
    clips = torch.zeros(2, 2, 3, 48, 48)
    for fn in (frame_patch_attention, patch_temporal_attention):
        with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
            fn(enc, clips)
        with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
            fn(holder, clips)                        # an AlproBaseModel stands for its visual_encoder
        with pytest.raises(ValueError, match=r"not \(B, T, C, H, W\)"):
            fn(enc.eval(), clips[0])
        enc.train()
    with pytest.raises(ValueError, match="reduce_heads"):
        frame_patch_attention(enc.eval(), clips, reduce_heads="max")
