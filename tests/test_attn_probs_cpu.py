"""CPU: the host side of the attention-probability output -- alpro_attn_probs' ABI surface and argument checks (every check sits in front of the
first HIP call, so placeholder addresses are never read), the self-check of the case builders (tests/attn_probs_cases.py), how BertModel
resolves output_attentions / output_hidden_states from its config, and the refusals of the wrapper and of text_to_patch_attention."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import attn_probs_cases as ac
from tests.conftest import BERT_CFG
from tests.test_host_cpu import make_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_entry_point_is_exported_and_declared_under_abi_22():
    from alpro_amd import hip
    hdr = open(os.path.join(ROOT, "include", "alpro_hip.h")).read()
    lib = hip.load()
    assert "alpro_attn_probs" in hip.EXPORTS and re.search(r"\bint\s+alpro_attn_probs\s*\(", hdr) and hasattr(lib, "alpro_attn_probs")
    assert "#define ALPRO_HIP_ABI_VERSION 22" in hdr and hip.ABI_VERSION == 22 == lib.alpro_hip_abi_version()
    assert "#define ALPRO_ATTN_MAX_L 1024" in hdr


def test_bad_arguments_are_refused_with_a_message_that_names_the_value():
    from alpro_amd import hip
    lib = hip.load()
    p = ctypes.c_void_p(4096)
    good = dict(qkv=p, lse=p, kb=None, out=p, dtype=hip.F16, batch=2, L=40, H=2, q0=0, nq=40, k0=0, nk=40)

    def call(**kw):
        a = dict(good, **kw)
        return lib.alpro_attn_probs(a["qkv"], a["lse"], a["kb"], a["out"], a["dtype"], a["batch"], a["L"], a["H"], 0.125, a["q0"], a["nq"], a["k0"], a["nk"], None)

    for kw, msg in ((dict(L=0, nq=0, nk=0), "L=0"), (dict(L=1025, nq=1025, nk=1025), "L=1025"), (dict(q0=8, nq=33), "q0=8 nq=33"),
                    (dict(k0=39, nk=2), "k0=39 nk=2"), (dict(q0=-1, nq=3), "q0=-1"), (dict(nq=0), "nq=0"), (dict(nk=0), "nk=0"),
                    (dict(k0=2147483647, nk=2), "k0=2147483647"), (dict(dtype=3), "dtype=3"), (dict(dtype=-1), "dtype=-1"),
                    (dict(lse=None), "null lse"), (dict(qkv=None), "null qkv"), (dict(out=None), "null out"), (dict(batch=0), "batch=0"), (dict(H=0), "H=0"),
                    (dict(out=ctypes.c_void_p(4096 + 4)), "16-byte aligned"), (dict(qkv=ctypes.c_void_p(4096 + 8)), "16-byte aligned")):
        rc = call(**kw)
        assert rc != 0, kw
        assert msg in lib.alpro_hip_last_error().decode(), (kw, lib.alpro_hip_last_error())


def test_wrapper_refuses_cpu_tensors():
    from alpro_amd import hip
    qkv, lse = torch.zeros(2 * 8, 3 * 2 * 64), torch.zeros(2, 2, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attn_probs(qkv, lse, 2, 8, 2, 0.125)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip.attn_probs(np.zeros((16, 384), dtype=np.float32), lse, 2, 8, 2, 0.125)


@pytest.mark.parametrize("dtype", ac.DTYPES)
def test_case_builders_hold_what_they_claim(dtype):
    for L in (1, 33, 65):
        c = ac.random_case(L, dtype)
        assert c.qkv.shape == (3 * L, 3 * 2 * 64) and c.qkv.dtype == np.float32
        assert np.array_equal(ac.round_to(c.qkv, dtype), c.qkv)                     # already representable in the operand dtype
        assert np.abs(c.p64.sum(axis=-1) - 1.0).max() < 1e-12                       # fp64 rows sum to 1
        assert np.abs(np.log(np.exp(c.s64 - c.lse64[..., None]).sum(-1))).max() < 1e-12
        assert c.bias.shape == (3, L) and set(np.unique(c.bias)) <= {np.float32(0.0), np.float32(-10000.0)}
        # all keys of sequence 2 masked: a constant bias cancels, the rows are the softmax of the bare scores, computed at s of about -10000
        assert (c.bias[2] == -10000.0).all() and (c.s64[2] < -9900).all()
        assert np.abs(c.p64[2:] - ac.softmax64(c.qkv, None, 3, L, 2, ac.SCALE)[1][2:]).max() < 1e-9
        if L > 4:
            assert (c.bias[0, -(L // 4):] == -10000.0).all() and c.p64[0, :, :, -(L // 4):].max() < 1e-300     # masked keys get nothing
            assert c.bias[1, L // 2] == -10000.0 and (np.delete(c.bias[1], L // 2) == 0).all()
        # the bound: above the floor everywhere, far below the probabilities it guards where they matter, and it grows with the lse error
        lim0 = ac.bound(c, np.zeros_like(c.lse64))
        assert (lim0 >= 2.0 ** -23).all() and (lim0 - 2.0 ** -23 <= c.p64 * 2e-3).all()
        assert (ac.bound(c, np.full_like(c.lse64, 1e-4)) >= lim0 + c.p64 * 9e-5).all()
        # check() accepts the fp64 answer rounded to fp32 and refuses a transposed map, a renormalised window and a value above 1
        p32, lse32 = c.p64.astype(np.float32), c.lse64.astype(np.float32)
        ac.check(c, p32, lse32)
        if L > 1:
            with pytest.raises(AssertionError):
                ac.check(c, np.ascontiguousarray(p32.transpose(0, 1, 3, 2)), lse32)
            bad = p32.copy()
            bad[0, 0, 0] *= np.float32(1.001)
            with pytest.raises(AssertionError):
                ac.check(c, bad, lse32)
    pk = ac.peaked_case(65, dtype)
    assert 55.0 < np.abs(pk.s64).max() < 70.0 and np.abs(pk.p64.sum(axis=-1) - 1.0).max() < 1e-12
    assert (pk.s64.max(axis=-1) > 50).all() and (pk.s64.min(axis=-1) < -50).all()


def test_output_flags_come_from_the_config_unless_given():
    from alpro_amd.modeling.xbert import BertModel
    small = dict(BERT_CFG, num_hidden_layers=2, fusion_layer=1, vocab_size=64, hidden_size=64, num_attention_heads=1, intermediate_size=128,
                 max_position_embeddings=16)
    m = BertModel(make_cfg(small), add_pooling_layer=False)
    assert m.output_flags() == (False, False)                                  # an attribute bag without the two fields: off
    assert m.output_flags(True, None) == (True, False) and m.output_flags(None, True) == (False, True)
    m = BertModel(make_cfg(small, output_attentions=True, output_hidden_states=False), add_pooling_layer=False)
    assert m.output_flags() == (True, False) and m.output_flags(False, True) == (False, True)   # an explicit argument wins (xbert.py:977-980)
    m = BertModel(make_cfg(small, output_attentions=False, output_hidden_states=True), add_pooling_layer=False)
    assert m.output_flags() == (False, True)
    # return_dict=False: the reference's tuple order, and the plain 1-tuple when nothing was asked for
    out, hs, at = object(), (1, 2), (3,)
    assert BertModel._result(out, None, None, False) == (out,)
    assert BertModel._result(out, hs, at, False) == (out, None, hs, at) and BertModel._result(out, None, at, False) == (out, None, at)
    r = BertModel._result(out, hs, None, True)
    assert r.last_hidden_state is out and r.hidden_states is hs and r.attentions is None


def test_text_to_patch_attention_refuses_a_model_in_train_mode():
    from alpro_amd.grounding import text_to_patch_attention
    m = torch.nn.Module().train()
    ids = torch.zeros(2, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match=r"model\.eval\(\)"):
        text_to_patch_attention(m, ids, torch.ones_like(ids), torch.zeros(2, 5, 64))
    with pytest.raises(ValueError, match="reduce_heads"):
        text_to_patch_attention(m.eval(), ids, torch.ones_like(ids), torch.zeros(2, 5, 64), reduce_heads="max")
    with pytest.raises(ValueError, match="square patch grid"):
        text_to_patch_attention(m.eval(), ids, torch.ones_like(ids), torch.zeros(2, 7, 64))
