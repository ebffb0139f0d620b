#!/usr/bin/env python3
"""Compare the gfx950 code of the same translation units in two build trees, kernel by kernel: the check for a refactor that must not change
machine code.

    python tools/obj_isa_diff.py [--ignore-addresses] OLD_OBJDIR NEW_OBJDIR attention.o attention_bwd.o ...

Each object's gfx950 code object is extracted (llvm-objdump --offloading); per kernel symbol it compares (a) the disassembly (llvm-objdump -d,
addresses and encodings included) and (b) the kernel's entry of the AMDGPU metadata note (llvm-readelf --notes: register counts, LDS and private
segment sizes, arguments).  Prints one line per object and one per differing kernel; exit status 1 on any difference.  CPU only.

--ignore-addresses: for a change that ADDS kernels to a translation unit and must leave the others as they are.  New kernels move the old ones
to other addresses, so the address column, the zero fill behind a function and the distance literal of a pc-relative reference to a global
(s_getpc_b64 + s_add_u32 / s_addc_u32) differ although every other instruction and encoding is the same (branch targets are printed relative to the
function's symbol).  With the flag those three are dropped before comparing, and symbols found only in the new object are listed without counting
as a difference.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=cwd).stdout


def code_object(obj, work):
    os.makedirs(work)
    shutil.copy(obj, work)
    run(os.path.join(LLVM, "llvm-objdump"), "--offloading", os.path.basename(obj), cwd=work)
    dev = [f for f in os.listdir(work) if "gfx950" in f]
    assert len(dev) == 1, os.listdir(work)
    return os.path.join(work, dev[0])


def kernels(co):
    """{kernel symbol: (disassembly text, metadata entry text)}; functions that are not kernels are keyed '<name> (function)'."""
    note = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    body = note.split("amdhsa.kernels:", 1)[1].split("\namdhsa.", 1)[0]
    meta = {}
    for entry in re.split(r"\n(?=  - \.)", body):
        m = re.search(r"^\s+\.name:\s+(\S+)", entry, re.M)
        if m:
            meta[m.group(1)] = entry
    dis = run(os.path.join(LLVM, "llvm-objdump"), "-d", co).split("\n", 2)[2]   # drop the file-name header line
    out = {}
    for fn in re.split(r"\n(?=[0-9a-f]{16} <)", dis):
        m = re.match(r"\s*[0-9a-f]{16} <(\S+)>:", fn)
        if m:
            name = m.group(1)
            out[name if name in meta else name + " (function)"] = (fn.strip(), meta.get(name, ""))
    assert set(meta) <= set(out), sorted(set(meta) - set(out))
    return out


def strip_addresses(text):
    lines = [re.sub(r"// [0-9A-F]+: ", "// ", ln) for ln in text.split("\n")]
    for i, ln in enumerate(lines):   # the literal of a pc-relative address of a global (s_getpc_b64, then s_add_u32 / s_addc_u32 with the distance)
        if "s_getpc_b64" in ln:
            for j in range(i + 1, min(i + 4, len(lines))):
                if re.match(r"\s*s_addc?_u32 .*, 0x[0-9a-f]+\s", lines[j]):
                    lines[j] = re.sub(r", 0x[0-9a-f]+\s.*$", ", <pc-relative distance>", lines[j])
    lines[0] = re.sub(r"^\s*[0-9a-f]{16} ", "", lines[0])
    while lines and (not lines[-1].strip() or lines[-1].strip() == "..." or lines[-1].strip().startswith("s_code_end")):
        lines.pop()
    return "\n".join(lines)


def main():
    args = sys.argv[1:]
    relaxed = "--ignore-addresses" in args
    args = [a for a in args if a != "--ignore-addresses"]
    old_dir, new_dir, names = args[0], args[1], args[2:]
    bad = False
    with tempfile.TemporaryDirectory() as tmp:
        for n in names:
            a = kernels(code_object(os.path.join(old_dir, n), os.path.join(tmp, "old_" + n)))
            b = kernels(code_object(os.path.join(new_dir, n), os.path.join(tmp, "new_" + n)))
            if relaxed:
                a = {k: (strip_addresses(d), m) for k, (d, m) in a.items()}
                b = {k: (strip_addresses(d), m) for k, (d, m) in b.items()}
            same_set = set(a) == set(b) or (relaxed and set(a) <= set(b))
            common = sorted(set(a) & set(b))
            dis_diff = [k for k in common if a[k][0] != b[k][0]]
            meta_diff = [k for k in common if a[k][1] != b[k][1]]
            insns = sum(len(re.findall(r"^\s+[sv]_|^\s+(ds|global|buffer|flat|scratch)_", a[k][0], re.M)) for k in common)
            print("%-28s kernels %3d   symbols identical %-3s   disassembly identical %-3s   metadata identical %-3s   (%d instructions compared)"
                  % (n, len(a), "yes" if same_set else "NO", "yes" if not dis_diff else "NO", "yes" if not meta_diff else "NO", insns))
            for k in sorted(set(a) ^ set(b)):
                print("    only in %s: %s" % ("old" if k in a else "new", k))
            for k in dis_diff:
                la, lb = a[k][0].split("\n"), b[k][0].split("\n")
                print("    disassembly differs: %s (%d vs %d lines)" % (k, len(la), len(lb)))
            for k in meta_diff:
                get = lambda e: {f: re.search(re.escape(f) + r":\s+(\S+)", e).group(1) for f in FIELDS}  # noqa: E731
                print("    metadata differs: %s old %s new %s" % (k, get(a[k][1]), get(b[k][1])))
            bad = bad or not same_set or bool(dis_diff) or bool(meta_diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
