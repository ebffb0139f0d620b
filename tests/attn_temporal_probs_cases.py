"""Cases for alpro_attn_temporal_probs (the temporal attention probabilities of the visual encoder).  Shared by tests/test_attn_temporal_probs_gpu.py
and tests/test_vit_attn_maps_cpu.py; not collected itself, numpy / torch on the CPU only.

A temporal problem over `groups` groups of T consecutive rows IS a problem of tests/attn_probs_cases.py with batch = groups, L = T and no key bias:
the q | k | v rows are the same (rows, 3*H*64) matrix, row g*T + t.  Only the log-sum-exp rows are laid out differently -- (batch, H, L) there,
((rows + 31) // 32, H, 32) here: row c*32 + r of head h at [c, h, r] -- so the cases, the fp64 expectation and the derived bound (check) are that
file's; this one adds the two re-layouts and the shape lists.
"""
import numpy as np

from tests import attn_probs_cases as ac

FRAMES = (1, 2, 3, 4, 5, 7, 8, 12, 16, 31, 32, 33, 48, 64, 127, 128)   # every T dividing 32 (the unit form), both sides of every 32-tile edge up to 4 x 4 tiles
GROUPS = (1, 5, 37)                                                    # rows = groups * T is no multiple of 32 (except at T = 32), groups straddle 32-row chunks
DTYPES = ac.DTYPES


def temporal_case(T, dtype, groups, H=2):
    return ac.random_case(T, dtype, batch=groups, H=H, bias="none")


def peaked_temporal_case(T, dtype, groups, H=2):
    return ac.peaked_case(T, dtype, batch=groups, H=H)


def case_from_qkv(name, qkv, groups, T, H, dtype, scale=ac.SCALE):
    """A case around q | k | v rows that a device kernel produced (fp32 numpy holding values of the operand dtype)."""
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    s, p, lse, ad = ac.softmax64(qkv, None, groups, T, H, scale)
    return ac.Case(name, groups, T, H, dtype, scale, qkv, None, s, p, lse, ad)


def lse_to_chunks(lse, fill=0.0):
    """(groups, H, T) -> ((rows + 31) // 32, H, 32), rows = groups * T: the layout alpro_attn_temporal_fwd writes; slots past the last row hold `fill`."""
    lse = np.asarray(lse)
    groups, H, T = lse.shape
    rows = groups * T
    chunks = (rows + 31) // 32
    flat = np.full((chunks * 32, H), fill, dtype=lse.dtype)
    flat[:rows] = lse.transpose(0, 2, 1).reshape(rows, H)
    return np.ascontiguousarray(flat.reshape(chunks, 32, H).transpose(0, 2, 1))


def lse_from_chunks(chunks, groups, T):
    """((rows + 31) // 32, H, 32) -> (groups, H, T)."""
    chunks = np.asarray(chunks)
    H = chunks.shape[1]
    rows = groups * T
    flat = chunks.transpose(0, 2, 1).reshape(-1, H)[:rows]
    return np.ascontiguousarray(flat.reshape(groups, T, H).transpose(0, 2, 1))
