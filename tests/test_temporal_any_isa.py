"""CPU: the built attention_temporal_any.o (temporal attention for frame counts that do not divide 32) keeps every kernel in registers -- no
scratch access -- and uses only the 32x32 MFMA forms of the other attention kernels: K = 16 for bf16 / f16, 32x32x2 for f32 (never
v_mfma_f32_16x16x16_*, whose P V rows came out wrong in one build: DESIGN.md section 0)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_temporal_any_isa(tmp_path):
    obj = os.path.join(ROOT, "alpro_amd", "lib", "obj", "attention_temporal_any.o")
    if not (os.path.exists(obj) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("needs the built attention_temporal_any.o (python -m alpro_amd.build) and llvm-objdump")
    work = tmp_path / "attention_temporal_any.o"
    shutil.copy(obj, work)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(work)], check=True, capture_output=True, cwd=tmp_path)
    dev = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert len(dev) == 1, os.listdir(tmp_path)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
    funcs = [f for f in re.split(r"\n(?=[0-9a-f]{16} <)", dis) if "tattn_any_" in f.split("\n", 1)[0]]
    names = [f.split("\n", 1)[0] for f in funcs]
    for kind in ("fwd", "bwd"):
        for dt in ("If", "bf16_t", "f16_t"):
            assert any("tattn_any_%s_kernel" % kind in n and dt in n for n in names), (kind, dt, names)
    for fn in funcs:
        head = fn.split("\n", 1)[0]
        assert "scratch_" not in fn and "buffer_store" not in fn, head
        mfma = set(re.findall(r"v_mfma_\w+", fn))
        assert mfma, head
        want = {"v_mfma_f32_32x32x2_f32"} if "kernelIf" in head else {"v_mfma_f32_32x32x16_bf16", "v_mfma_f32_32x32x16_f16"}
        assert mfma <= want, (head, mfma)
