#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds:  kernel_diff.py DIR_A DIR_B

DIR_A and DIR_B hold the objects (*.o) or libraries (*.so) of two builds of torch_nf_amd/csrc.  For every file the
device code objects are taken out of the .hip_fatbin section (clang offload bundles), and for every kernel its name,
its size, a hash of its machine code in .text and its 64-byte kernel descriptor (<name>.kd) are tabulated.  One field
of the descriptor, the distance from the descriptor to the code, moves with the order in which the host code
instantiates the kernels: it is checked to lead to the kernel's own code and then left out of the comparison.
Kernels that differ between the two sides are printed; the exit status is 0 only if there is none.  A host-side
refactor must leave the two tables equal -- whole-file hashes are no test, they differ even when every kernel is
identical.  The files are only read and hashed, never executed."""
import hashlib
import os
import struct
import sys

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def elf_sections(b):
    assert b[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64"
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    secs = []
    for i in range(shnum):
        name, typ, _, addr, off, size, link, _, _, entsize = struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize)
        secs.append(dict(name=name, type=typ, addr=addr, off=off, size=size, link=link, entsize=entsize))
    strtab = secs[shstrndx]
    for s in secs:
        end = b.index(b"\0", strtab["off"] + s["name"])
        s["name"] = b[strtab["off"] + s["name"]:end].decode()
    return secs


def code_objects(host):
    """the gfx950 code objects inside a host object's / library's .hip_fatbin section"""
    out = []
    for s in elf_sections(host):
        if s["name"] != ".hip_fatbin":
            continue
        fat = host[s["off"]:s["off"] + s["size"]]
        assert b"CCOB" not in fat[:4], "compressed offload bundle: build without --offload-compress"
        pos = fat.find(MAGIC)
        while pos >= 0:
            n, = struct.unpack_from("<Q", fat, pos + len(MAGIC))
            p = pos + len(MAGIC) + 8
            for _ in range(n):
                off, size, tlen = struct.unpack_from("<QQQ", fat, p)
                triple = fat[p + 24:p + 24 + tlen].decode()
                p += 24 + tlen
                if "gfx950" in triple and size:
                    out.append(fat[pos + off:pos + off + size])
            pos = fat.find(MAGIC, p)
    return out


def kernel_table(co):
    """{kernel name: (code size, sha256 of its code, hex of its descriptor)} of one code object"""
    secs = elf_sections(co)
    syms = {}
    for s in secs:
        if s["type"] != 2:  # SHT_SYMTAB
            continue
        strs = secs[s["link"]]["off"]
        for i in range(s["size"] // 24):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", co, s["off"] + 24 * i)
            if 0 < shndx < len(secs):
                end = co.index(b"\0", strs + name)
                sec = secs[shndx]
                syms[co[strs + name:end].decode()] = (value, co[sec["off"] + value - sec["addr"]:][:size])
    table = {}
    for name, (kd_addr, kd) in syms.items():
        if name.endswith(".kd") and name[:-3] in syms:
            assert len(kd) == 64, name
            addr, code = syms[name[:-3]]
            # bytes 16..23 hold the distance from the descriptor to the code: where the linker put the two, not what the
            # kernel is.  It must lead to the kernel's own code; it is then left out of the comparison.
            entry, = struct.unpack_from("<q", kd, 16)
            assert kd_addr + entry == addr, name + ": descriptor does not point at its code"
            table[name[:-3]] = (len(code), hashlib.sha256(code).hexdigest(), (kd[:16] + kd[24:]).hex())
    return table


def build_table(d):
    table = {}
    for f in sorted(os.listdir(d)):
        if f.endswith((".o", ".so")):
            with open(os.path.join(d, f), "rb") as fh:
                for co in code_objects(fh.read()):
                    for k, v in kernel_table(co).items():
                        table[(f, k)] = v
    return table


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = build_table(sys.argv[1]), build_table(sys.argv[2])
    bad = 0
    for key in sorted(set(a) | set(b)):
        if a.get(key) == b.get(key):
            continue
        bad += 1
        va, vb = a.get(key), b.get(key)
        what = "only in A" if vb is None else "only in B" if va is None else \
            ", ".join(n for n, x, y in zip(("size", "code", "descriptor"), va, vb) if x != y) + " differ"
        print("%s: %s: %s" % (key[0], key[1], what))
    files = len({f for f, _ in a} | {f for f, _ in b})
    print("%d files, %d kernels in A, %d in B, %d differ" % (files, len(a), len(b), bad))
    return 1 if bad or not a else 0


if __name__ == "__main__":
    sys.exit(main())
