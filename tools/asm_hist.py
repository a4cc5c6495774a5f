#!/usr/bin/env python3
"""Static instruction histogram of one kernel in a gfx950 listing (hipcc with the flags of build.py plus --cuda-device-only -S).
Prints the totals by unit (scalar, vector, MFMA, memory / LDS, other), the register and scratch figures of the kernel's metadata and the
most frequent mnemonics.
usage: asm_hist.py <listing.s> <substring of the mangled kernel name> [top=16]
   e.g. asm_hist.py nn1_brute.s nn1_strack3_kernelILi1E"""
import collections, re, sys


def kernel_body(lines, key):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and key in l)
    # to the end of the FUNCTION (.Lfunc_end<n>: / .size), not to the first s_endpgm: a kernel whose surplus waves leave early has one near its top
    end = next(i for i in range(start, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[i]) or lines[i].lstrip().startswith(".size"))
    meta = {}
    for l in lines[start:]:                      # (the kernel's descriptor block stands in front of .Lfunc_end, behind the last instruction)
        m = re.match(r"\s*\.(vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count):?\s+(\w+)", l) or \
            re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size|group_segment_fixed_size)\s+(\w+)", l)
        if m and m.group(1) not in meta:
            meta[m.group(1)] = m.group(2)
        if l.lstrip().startswith(".end_amdhsa_kernel"):
            break
    return lines[start + 1:end], meta


def unit(op):
    if "mfma" in op:
        return "mfma"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_", "ds_", "s_load", "s_buffer_load")):
        return "memory/lds"
    if op.startswith("v_"):
        return "vector"
    if op.startswith(("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_endpgm", "s_barrier", "s_sleep", "s_setprio")):
        return "other"
    if op.startswith("s_"):
        return "scalar"
    return "other"


def main():
    lines = open(sys.argv[1]).read().splitlines()
    body, meta = kernel_body(lines, sys.argv[2])
    top = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    ops = [l.split()[0] for l in body if l.startswith("\t") and not l.lstrip().startswith((".", ";")) and l.split()]
    hist = collections.Counter(ops)
    units = collections.Counter(unit(o) for o in ops)
    print(f"{sys.argv[2]}: {len(ops)} static instructions:", ", ".join(f"{k} {v}" for k, v in units.most_common()))
    print("  ", " ".join(f"{k}={v}" for k, v in meta.items()))
    print("  ", " ".join(f"{k} {v}" for k, v in hist.most_common(top)))


if __name__ == "__main__":
    main()
