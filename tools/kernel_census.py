#!/usr/bin/env python3
"""Census of the compiled gfx950 kernels: one line per kernel -- source, mangled name, code size, sha256 of its code bytes.

    python tools/kernel_census.py [-o listing.txt] [source.hip ...]

Every .hip of build.py's SOURCES (or the ones named) is compiled device-only with FLAGS + its SOURCE_FLAGS, the gfx950 code
object is unbundled, and the kernels (the FUNC symbols that own a <name>.kd descriptor) are read from its ELF symbol table.
Nothing is disassembled.  Two listings of two commits compare with diff(1): the same lines = the same device code.
The totals per source go to stderr.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from iq_tool_amd import build as B  # noqa: E402

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def llvm_tool(name):
    return os.path.join(os.path.dirname(os.path.realpath(B.hipcc())), "..", "llvm", "bin", name)


def census(sname, tmp):
    """[(name, size, sha256)] of one source's kernels, sorted by name"""
    obj, co = os.path.join(tmp, sname + ".o"), os.path.join(tmp, sname + ".co")
    subprocess.run([B.hipcc(), *B.FLAGS, *B.SOURCE_FLAGS.get(sname, []), "--cuda-device-only", "-c", sname, "-o", obj], check=True, cwd=B.CSRC)
    subprocess.run([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + obj, "--targets=" + TARGET, "--output=" + co], check=True)
    text = subprocess.run([llvm_tool("llvm-readelf"), "-S", "-s", "-W", co], check=True, capture_output=True, text=True).stdout
    # section headers: [Nr] Name Type Address Off Size ...;  symbols: Num: Value Size Type Bind Vis Ndx Name
    sections = {int(m[1]): (int(m[2], 16), int(m[3], 16)) for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s", text, re.M)}
    symtab = text[text.index("Symbol table '.symtab'"):]
    syms = {m[5]: (int(m[1], 16), int(m[2]), m[3], m[4]) for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]{16})\s+(\d+)\s+(\w+)\s+\w+\s+\w+\s+(\d+)\s+(\S+)$", symtab, re.M)}
    blob = open(co, "rb").read()
    rows = []
    for name, (addr, size, kind, ndx) in syms.items():
        if kind == "FUNC" and name + ".kd" in syms:
            sh_addr, sh_off = sections[int(ndx)]
            code = blob[addr - sh_addr + sh_off:][:size]
            assert len(code) == size, name
            rows.append((name, size, hashlib.sha256(code).hexdigest()))
    return sorted(rows)


def main(argv):
    out = sys.stdout
    if argv[:1] == ["-o"]:
        out, argv = open(argv[1], "w"), argv[2:]
    sources = argv or [s for s in B.SOURCES if s.endswith(".hip")]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(6, max(1, (os.cpu_count() or 2) - 1))) as ex:
        per_source = list(ex.map(lambda s: census(s, tmp), sources))
    n_all = b_all = 0
    for sname, rows in zip(sources, per_source):
        for name, size, digest in rows:
            print(sname, name, size, digest, file=out)
        print("%-18s %4d kernels %9d bytes" % (sname, len(rows), sum(r[1] for r in rows)), file=sys.stderr)
        n_all, b_all = n_all + len(rows), b_all + sum(r[1] for r in rows)
    print("%-18s %4d kernels %9d bytes" % ("total", n_all, b_all), file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1:])
