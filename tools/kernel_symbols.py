#!/usr/bin/env python3
"""List the kernel symbols of a library's gfx950 code objects, one mangled
name per line, sorted (a kernel is a symbol with a `.kd` descriptor).

  python tools/kernel_symbols.py fpn-mt-image-captioning_amd/fpnmt/libfpnmt.so > kernels.txt

Walks every clang offload bundle in the file (one per translation unit),
takes the entries whose target ends in the architecture and reads their symbol
tables with llvm-readelf. Used for profiles/dispatch_plan/: which kernel
instantiations a change of the dispatch adds or removes.
"""
import os
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
READELF = os.environ.get("LLVM_READELF", "/opt/rocm/llvm/bin/llvm-readelf")


def code_objects(blob, arch):
    pos = blob.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", blob, pos + len(MAGIC))
        at = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, at)
            triple = blob[at + 24:at + 24 + tlen].decode()
            at += 24 + tlen
            if triple.endswith(arch) and size:
                yield blob[pos + off:pos + off + size]
        pos = blob.find(MAGIC, pos + 1)


def main():
    path, arch = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "gfx950")
    names = []
    with open(path, "rb") as f:
        blob = f.read()
    for co in code_objects(blob, arch):
        with tempfile.NamedTemporaryFile(suffix=".co") as t:
            t.write(co)
            t.flush()
            out = subprocess.run([READELF, "--symbols", "--wide", t.name], check=True, capture_output=True, text=True).stdout
        mine = set()  # .dynsym and .symtab list a kernel once each
        for line in out.splitlines():
            cols = line.split()
            if len(cols) == 8 and cols[7].endswith(".kd"):
                mine.add(cols[7][:-3])
        names += mine  # a kernel instantiated in two translation units is listed twice
    print("\n".join(sorted(names)))


if __name__ == "__main__":
    main()
