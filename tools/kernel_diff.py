#!/usr/bin/env python3
"""Compares the kernels of two device-only gfx950 objects of one source file: per kernel symbol the bytes of the function and the kernel's
entry in the code object's metadata (registers, LDS, scratch, spills, arguments).  The 64-byte .kd descriptors are not compared: they hold
the code offset, which moves when any function in front of the kernel changes size.

  hipcc <the Makefile's FLAGS> --cuda-device-only --no-gpu-bundle-output -c edit.hip -o edit.dev.o      (once per revision)
  tools/kernel_diff.py parent/edit.dev.o tree/edit.dev.o

Prints one line per kernel of either object and a summary; needs llvm-readelf (ROCm: /opt/rocm/llvm/bin) and PyYAML."""
import hashlib
import os
import subprocess
import sys

import yaml

READELF = os.environ.get("LLVM_READELF", "/opt/rocm/llvm/bin/llvm-readelf")
FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def kernels(path):
    """name -> (sha1 of the function's bytes, size, metadata entry)"""
    data = open(path, "rb").read()
    text = subprocess.check_output([READELF, "-S", "-s", "-W", path], text=True)
    sections, funcs = {}, {}
    for line in text.splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) >= 6 and f[0].isdigit() and f[2] in ("PROGBITS", "NOBITS", "NOTE", "STRTAB", "SYMTAB", "DYNSYM", "HASH", "GNU_HASH", "DYNAMIC", "RELA", "REL"):
            sections[int(f[0])] = (int(f[3], 16), int(f[4], 16))                 # address, file offset
        elif len(f) == 8 and f[0].endswith(":") and f[3] == "FUNC" and f[6].isdigit():
            funcs[f[7]] = (int(f[1], 16), int(f[2]), int(f[6]))                  # value, size, section
    notes = subprocess.check_output([READELF, "--notes", path], text=True)
    doc = notes[notes.index("---"):notes.index("...", notes.index("---"))]
    out = {}
    for k in yaml.safe_load(doc)["amdhsa.kernels"]:
        name = k[".name"]
        value, size, sec = funcs[name]
        addr, off = sections[sec]
        body = data[off + value - addr: off + value - addr + size]
        out[name] = (hashlib.sha1(body).hexdigest(), size, k)
    return out


def demangle(names):
    try:
        res = subprocess.check_output(["c++filt"] + names, text=True).splitlines()
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(set(a) | set(b))
    nice = demangle(names)
    same = changed = 0
    for n in names:
        short = nice[n].split("(")[0].replace("void ", "")
        fig = lambda k: " ".join("%s=%s" % (f[1:].replace("_count", "").replace("_segment_fixed_size", ""), k.get(f, 0)) for f in FIGURES)
        if n not in a or n not in b:                     # (a kernel whose parameter list changed has another symbol: it shows as one line of each kind)
            k = a[n] if n in a else b[n]
            print("%-32s only in the %s: %6d bytes  %s" % (short, "first" if n in a else "second", k[1], fig(k[2])))
            continue
        code_same, meta_same = a[n][0] == b[n][0], a[n][2] == b[n][2]
        if code_same and meta_same:
            same += 1
            print("%-32s identical: %6d bytes  %s" % (short, a[n][1], fig(a[n][2])))
        else:
            changed += 1
            print("%-32s CHANGED: code %s (%d -> %d bytes), metadata %s" % (short, "same" if code_same else "differs", a[n][1], b[n][1], "same" if meta_same else "differs"))
            print("%-32s   first:  %s" % ("", fig(a[n][2])))
            print("%-32s   second: %s" % ("", fig(b[n][2])))
    print("%d kernels identical in code and metadata, %d changed, %d only in the first, %d only in the second"
          % (same, changed, len([n for n in names if n not in b]), len([n for n in names if n not in a])))


if __name__ == "__main__":
    main()
