#!/usr/bin/env python3
"""Which sim_kernel instantiations differ between two builds of libdash.so, counted per MODE.

Usage: python3 tools/fingerprint_modes.py PARENT/libdash.so [libdash.so]
Every `sim_kernel<P, CS, RING, MODE>` of both libraries is fingerprinted with tools/kernel_fingerprint.py
(code bytes and descriptor); the two must hold the same instantiations. One line per MODE: how many are
byte-identical and how many changed. Needs no GPU: a cross-compiled build of each commit will do."""
import pathlib
import re
import struct
import sys

import kernel_fingerprint as kf


def sim_kernels(lib):
    elf = kf.code_object(pathlib.Path(lib).read_bytes())
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    out = set()
    for sh in secs:
        if sh[1] != 2:  # SHT_SYMTAB
            continue
        strtab = secs[sh[6]]
        for k in range(sh[5] // 24):
            st_name, = struct.unpack_from("<I", elf, sh[4] + k * 24)
            s = elf[strtab[4] + st_name:elf.index(b"\0", strtab[4] + st_name)].decode()
            if s.startswith("_ZN4dash10sim_kernelI") and s.endswith("SimArgsE"):
                out.add(s)
    return out


def compare(parent, tree=kf.LIB):
    syms = sim_kernels(parent)
    assert syms == sim_kernels(tree), "the builds hold different instantiations"
    modes = {}
    for s in sorted(syms):
        mode = int(re.search(r"ELi(\d+)EEEv", s).group(1))
        same = kf.fingerprint(parent, s) == kf.fingerprint(tree, s)
        modes.setdefault(mode, [0, 0])[0 if same else 1] += 1
    return modes


if __name__ == "__main__":
    for mode, (same, changed) in sorted(compare(*sys.argv[1:3]).items()):
        print(f"MODE {mode}: {same} identical, {changed} changed")
