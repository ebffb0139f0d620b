"""CPU: the built attention_long.o (the L > 256 attention kernels) keeps every kernel in registers -- no scratch access -- and uses only the K = 16
32x32 MFMA forms the whole-row kernels use (never v_mfma_f32_16x16x16_*, whose P V rows came out wrong in one build: DESIGN.md section 0)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_attention_long_isa(tmp_path):
    obj = os.path.join(ROOT, "alpro_amd", "lib", "obj", "attention_long.o")
    if not (os.path.exists(obj) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("needs the built attention_long.o (python -m alpro_amd.build) and llvm-objdump")
    work = tmp_path / "attention_long.o"
    shutil.copy(obj, work)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(work)], check=True, capture_output=True, cwd=tmp_path)
    dev = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert len(dev) == 1, os.listdir(tmp_path)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
    funcs = [f for f in re.split(r"\n(?=[0-9a-f]{16} <)", dis) if "attn_long_" in f.split("\n", 1)[0]]
    names = [f.split("\n", 1)[0] for f in funcs]
    for kind in ("fwd", "cls", "dq", "dkv"):
        assert any("attn_long_%s_kernel" % kind in n for n in names), (kind, names)
    for fn in funcs:
        head = fn.split("\n", 1)[0]
        assert "scratch_" not in fn and "buffer_store" not in fn, head
        assert not re.search(r"v_mfma_f32_16x16x16", fn), head
        if "cls_kernel" not in head:
            assert re.search(r"v_mfma_f32_32x32x(16_bf16|16_f16|2_?f32)", fn), head
