#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libgptsgld.so, symbol by symbol.

    python scripts/compare_isa.py BASE.so CANDIDATE.so [--llvm /opt/rocm/llvm/bin]

For a host-only change the two libraries must hold the same device code.  Each library's
.hip_fatbin section is a run of offload bundles (one per translation unit); the gfx950 code object
of every bundle is disassembled and its metadata note read.  Compared, per translation unit:
the set of function symbols, each function's instruction text, and each kernel's metadata entry
(register counts, spills, private and group segment sizes, arguments).  The order of the functions
inside a code object may differ; nothing else may.  Exit status 0 when nothing differs.
"""
import argparse
import re
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_objects(lib, llvm, tmp):
    """The gfx950 code object of every offload bundle of lib, in link order."""
    fat = tmp / (Path(lib).name + ".fatbin")
    run(str(llvm / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(lib), str(tmp / "x"))
    data = fat.read_bytes()
    out = []
    for m in re.finditer(MAGIC, data):
        base = m.start()
        (count,) = struct.unpack_from("<Q", data, base + len(MAGIC))
        pos = base + len(MAGIC) + 8
        for _ in range(count):
            off, size, idlen = struct.unpack_from("<QQQ", data, pos)
            ident = data[pos + 24:pos + 24 + idlen].decode()
            pos += 24 + idlen
            if "gfx950" in ident and size:
                out.append(data[base + off:base + off + size])
    return out


def symbols(co, llvm):
    """[(address, size, name)] of a code object's functions and data objects."""
    out = set()
    for line in run(str(llvm / "llvm-readelf"), "-sW", str(co)).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6] != "UND":
            out.add((int(f[1], 16), int(f[2]), f[7]))
    return sorted(out)


def functions(co, llvm):
    """{symbol: instruction text} of a code object, independent of where the functions lie: the
    padding after a function's last instruction is dropped, and the literal of a pc-relative
    address (s_getpc_b64, then s_add_u32 with the distance) is replaced by the symbol it reaches."""
    syms = symbols(co, llvm)

    def where(addr):
        for a, size, name in syms:
            if a <= addr < a + max(size, 1):
                return "<%s+%#x>" % (name, addr - a)
        return "<unresolved %#x>" % addr

    text = run(str(llvm / "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", str(co))
    funcs, name, getpc = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            name = m.group(1)
            funcs[name] = []
            continue
        m = re.match(r"^\s+(\S.*?)\s*// ([0-9A-F]+):", line)
        if name is None or not m:
            continue
        ins, addr = m.group(1), int(m.group(2), 16)
        lit = re.match(r"(s_add_u32 \S+ \S+) 0x([0-9a-f]+)$", ins)
        if getpc is not None and lit:
            d = int(lit.group(2), 16)
            ins = "%s %s" % (lit.group(1), where(getpc + 4 + (d - (1 << 32) if d >> 31 else d)))
        getpc = addr if ins.startswith("s_getpc_b64") else None
        funcs[name].append(ins)
    for v in funcs.values():
        while v and v[-1] == "s_nop 0":
            v.pop()
    return {k: "\n".join(v) for k, v in funcs.items()}


def kernel_notes(co, llvm):
    """{kernel: its entry of the amdhsa.kernels metadata, as text}."""
    text = run(str(llvm / "llvm-readelf"), "--notes", str(co))
    m = re.search(r"^amdhsa\.kernels:\n(.*?)(?=^\S)", text, re.S | re.M)
    notes = {}
    for entry in re.split(r"(?m)^  - (?=\.)", m.group(1) if m else "")[1:]:
        notes[re.search(r"\.name:\s+(\S+)", entry).group(1)] = entry
    return notes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base")
    ap.add_argument("candidate")
    ap.add_argument("--llvm", default="/opt/rocm/llvm/bin")
    a = ap.parse_args()
    llvm = Path(a.llvm)
    nsym = nkern = 0
    diffs = []
    with tempfile.TemporaryDirectory() as d:
        tmp = Path(d)
        cos = [code_objects(lib, llvm, tmp) for lib in (a.base, a.candidate)]
        if len(cos[0]) != len(cos[1]):
            diffs.append(f"code objects: {len(cos[0])} vs {len(cos[1])}")
        for i, pair in enumerate(zip(*cos)):
            f, k = [], []
            for side, blob in enumerate(pair):
                p = tmp / f"co{i}_{side}.o"
                p.write_bytes(blob)
                f.append(functions(p, llvm))
                k.append(kernel_notes(p, llvm))
            nsym += len(f[0])
            nkern += len(k[0])
            for what, x in (("function", f), ("kernel note", k)):
                for s in sorted(set(x[0]) ^ set(x[1])):
                    diffs.append(f"unit {i}: {what} {s} only in {'base' if s in x[0] else 'candidate'}")
                for s in sorted(set(x[0]) & set(x[1])):
                    if x[0][s] != x[1][s]:
                        diffs.append(f"unit {i}: {what} {s} differs")
    print(f"code objects (translation units): {len(cos[0])}")
    print(f"function symbols compared: {nsym}")
    print(f"kernels compared (instruction text and metadata note): {nkern}")
    print(f"differences: {len(diffs)}")
    for s in diffs:
        print("  " + s)
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
