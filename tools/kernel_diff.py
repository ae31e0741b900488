#!/usr/bin/env python
"""Is the gfx950 device code of two builds of the library the same?   tools/kernel_diff.py OLD.so NEW.so
Extracts the code objects the way tests/test_kernel_resources.py does (llvm-objdump --offloading) and compares, per kernel name,
the metadata notes (registers, spills, private / group segment, workgroup size) and the disassembly without its address and
encoding columns.  The one difference let through is the literal of a pc-relative address (the s_add_u32 / s_addc_u32 pair behind
an s_getpc_b64), which moves when a constant table lands at another offset of its code object; they are counted.
Prints what differs and one summary line; exit status 1 unless the two are the same."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "sgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size")


def _normalise(lines):
    """the instruction text of one symbol; returns (text, number of pc-relative literals replaced)"""
    out, n, pair, left = [], 0, None, 0
    for line in lines:
        ins = re.sub(r"\s*//.*$", "", line).strip()         # (the comment holds the address and the encoding)
        if not ins:
            continue
        m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", ins)
        if m:
            pair, left = (m.group(1), m.group(2)), 6
        elif pair and left > 0:
            left -= 1
            a = re.match(r"(s_add_u32 s%s, s%s, )\S+$" % (pair[0], pair[0]), ins) or re.match(r"(s_addc_u32 s%s, s%s, )\S+$" % (pair[1], pair[1]), ins)
            if a:
                ins, n = a.group(1) + "<pcrel>", n + 1
        out.append(ins)
    while out and out[-1] in ("s_nop 0", "s_code_end", "..."):       # alignment padding up to the next symbol, not the kernel's
        out.pop()
    return "\n".join(out), n


def read_library(so):
    """({kernel: {field: value}}, {symbol: set of instruction texts}, pc-relative literals normalised)"""
    objdump, readelf = os.path.join(LLVM, "llvm-objdump"), os.path.join(LLVM, "llvm-readelf")
    tmp = tempfile.mkdtemp()
    try:
        lib = os.path.join(tmp, "lib.so")
        shutil.copy(so, lib)
        subprocess.run([objdump, "--offloading", lib], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        meta, text, npc = {}, {}, 0
        for co in sorted(glob.glob(os.path.join(tmp, "lib.so.*gfx950*"))):
            notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in notes.split("- .agpr_count:")[1:]:
                block = ".agpr_count:" + block
                name = re.search(r"\.name:\s+(\S+)", block)
                if name:
                    vals = {}
                    for k in FIELDS:
                        m = re.search(r"\.%s:\s+(\d+)" % k, block)
                        vals[k] = int(m.group(1)) if m else None
                    assert name.group(1) not in meta, "kernel %s in two code objects" % name.group(1)
                    meta[name.group(1)] = vals
            dis = subprocess.run([objdump, "-d", co], check=True, capture_output=True, text=True).stdout
            sym, lines = None, []
            for line in dis.split("\n") + ["0 <end>:"]:
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    if sym is not None:
                        t, n = _normalise(lines)
                        text.setdefault(sym, set()).add(t)
                        npc += n
                    sym, lines = m.group(1), []
                elif sym is not None:
                    lines.append(line)
        return meta, text, npc
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(old, new):
    (m0, t0, p0), (m1, t1, p1) = read_library(old), read_library(new)
    only0, only1 = sorted(set(m0) - set(m1)), sorted(set(m1) - set(m0))
    for k in only0:
        print("only in OLD: %s" % k)
    for k in only1:
        print("only in NEW: %s" % k)
    both = sorted(set(m0) & set(m1))
    bad_meta = [k for k in both if m0[k] != m1[k]]
    for k in bad_meta:
        print("metadata differs: %s: %s" % (k, {f: (m0[k][f], m1[k][f]) for f in FIELDS if m0[k][f] != m1[k][f]}))
    # every symbol with code: the kernels, and any device function that was not inlined
    syms = sorted(set(t0) | set(t1))
    bad_text = [s for s in syms if t0.get(s) != t1.get(s)]
    for s in bad_text:
        a, b = sorted(t0.get(s, [""]))[0].split("\n"), sorted(t1.get(s, [""]))[0].split("\n")
        i = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
        print("instruction text differs: %s: %d / %d instructions, first at %d: %r / %r" % (s, len(a), len(b), i, a[i:i + 1], b[i:i + 1]))
    n_ins = sum(len(x.split("\n")) for s in t1 for x in t1[s])
    same = not (only0 or only1 or bad_meta or bad_text)
    print("kernel_diff: %s: %d kernels in both (%d only in OLD, %d only in NEW), metadata differs in %d, instruction text differs in %d of %d symbols "
          "(%d instructions); pc-relative literals normalised: %d in OLD, %d in NEW" %
          ("IDENTICAL" if same else "DIFFERENT", len(both), len(only0), len(only1), len(bad_meta), len(bad_text), len(syms), n_ins, p0, p1))
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
