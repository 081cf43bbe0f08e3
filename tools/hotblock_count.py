#!/usr/bin/env python3
"""Instruction classes in the largest basic block of a kernel, and the registers of every kernel, from device assembly.

  hipcc -O3 -std=c++17 -fno-slp-vectorize --offload-arch=gfx950 --cuda-device-only -S \\
        torch_nf_amd/csrc/flow_fused2.hip -o ff2.s
  python tools/hotblock_count.py ff2.s [substring of the mangled kernel name]

The default kernel is the headline instance flow_fused2_kernel<32, 2, 2, 8, 4, false, false, ...>:
its largest block is one group of the main loop, 2 tiles x 8 layers.  Needs no GPU."""
import collections
import re
import sys

CLASSES = [("all instructions", r"."), ("v_mfma", r"v_mfma"), ("ds_read_b128", r"ds_read_b128"),
           ("v_exp / v_rcp", r"v_(exp|rcp)_f32"), ("v_cvt_pk_f16_f32", r"v_cvt_pk_f16_f32"),
           ("v_fma_mix_f32", r"v_fma_mix_f32"), ("v_fma / v_fmac", r"v_(fma|fmac)_f32"), ("v_mul", r"v_mul_f32"),
           ("v_mov_b32", r"v_mov_b32"), ("v_add_f32", r"v_add_f32")]


def kernels(text):
    """name -> list of basic blocks (lists of instruction mnemonics)"""
    out = {}
    cur = None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [[]])
            continue
        if cur is None:
            continue
        if re.match(r"^\s*\.end_amdhsa_kernel|^\.Lfunc_end", line):
            cur = None
            continue
        if re.match(r"^\.LBB\w+:", line):
            cur.append([])
            continue
        m = re.match(r"^\s+([a-z]\w+)", line)
        if m and not line.lstrip().startswith("."):
            cur[-1].append(m.group(1))
            if m.group(1).startswith(("s_cbranch", "s_branch")):
                cur.append([])
    return out


def resources(text):
    """name -> {vgpr_count, vgpr_spill_count, private_segment_fixed_size} from the metadata"""
    out = {}
    for blk in re.split(r"\n\s+- \.agpr_count", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        out[name.group(1)] = {k: get(k) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    return out


def main():
    text = open(sys.argv[1]).read()
    want = sys.argv[2] if len(sys.argv) > 2 else "flow_fused2_kernelILi32ELi2ELi2ELi8ELi4ELb0ELb0E"
    ks = kernels(text)
    for name, blocks in ks.items():
        if want not in name:
            continue
        hot = max(blocks, key=len)
        print(name)
        for label, pat in CLASSES:
            print("  %-18s %5d" % (label, sum(1 for i in hot if re.match(pat, i))))
        valu = collections.Counter(i for i in hot if i.startswith("v_") and not i.startswith("v_mfma"))
        print("  %-18s %5d" % ("vector, not MFMA", sum(valu.values())))
    print("%-100s vgpr spill scratch" % "kernel")
    for name, r in sorted(resources(text).items()):
        print("%-100s %4d %5d %7d" % (name[:100], r["vgpr_count"], r["vgpr_spill_count"], r["private_segment_fixed_size"]))


if __name__ == "__main__":
    main()
