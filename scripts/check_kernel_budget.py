#!/usr/bin/env python3
"""Build-time resource budget of one kernel, read from the metadata of the generated assembly.

    check_kernel_budget.py kernels.s [--kernel k_chain_potrf] [--max-regs 128]
                                     [--max-scratch 0] [--max-lds 81920]

The panel chain's POTRF launch is one workgroup that has to find room on a CU which another
stream keeps full of update workgroups.  A retiring k_update<64,16,2,2> workgroup frees
96 + 32 = 128 registers per lane per SIMD; a kernel that needs more is only placed when that
launch runs out of pending workgroups.  So the build fails when the kernel
grows past that hole.

Only the counts in the amdhsa.kernels metadata are read, no instruction:
  .vgpr_count                  registers per lane as allocated.  On gfx90a and later (one
                               unified file) this is the total, the accumulation registers
                               (.agpr_count) included; the line printed shows both.
  .private_segment_fixed_size  scratch bytes per lane (spills)
  .group_segment_fixed_size    static LDS bytes per workgroup (k_chain_potrf takes its LDS
                               dynamically, sizeof(PotrfShared), bounded by a static_assert at
                               its launch; a static allocation coming back is bounded here)
Exit status 0: within budget; 1: over budget; 2: kernel or a field not found.
"""
import argparse
import re
import sys

FIELDS = ("vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernel_entries(text):
    """The entries of amdhsa.kernels as dicts of their scalar 'key: value' lines."""
    start = text.find("amdhsa.kernels:")
    if start < 0:
        return []
    entries, cur = [], None
    for line in text[start:].splitlines()[1:]:
        if re.match(r"^\S", line):          # next top-level key (amdhsa.target, ...) or end marker
            break
        m = re.match(r"^  - \.(\w+):\s*(.*)$", line)
        if m:
            cur = {}
            entries.append(cur)
        else:
            m = re.match(r"^    \.(\w+):\s*(.*)$", line)
        if m and cur is not None and m.group(2) != "":
            cur[m.group(1)] = m.group(2).strip().strip("'\"")
    return entries


def check(text, kernel, max_regs, max_scratch, max_lds):
    """(status, message) for the one kernel whose .name contains `kernel`."""
    hits = [e for e in kernel_entries(text) if kernel in e.get("name", "")]
    if len(hits) != 1:
        return 2, f"{kernel}: {len(hits)} kernels of that name in the metadata"
    e = hits[0]
    try:
        regs, agpr, scratch, lds = (int(e[f]) for f in FIELDS)
    except (KeyError, ValueError) as err:
        return 2, f"{kernel}: metadata field {err} missing or not a number"
    msg = (f"{e['name']}: {regs} registers per lane ({regs - agpr} + {agpr} accumulation; budget {max_regs}), "
           f"{scratch} B scratch (budget {max_scratch}), {lds} B static LDS (budget {max_lds})")
    over = []
    if regs > max_regs:
        over.append("registers")
    if scratch > max_scratch:
        over.append("scratch")
    if lds > max_lds:
        over.append("LDS")
    if over:
        return 1, msg + "\nOVER BUDGET: " + ", ".join(over)
    return 0, msg


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="k_chain_potrf")
    ap.add_argument("--max-regs", type=int, default=128)
    ap.add_argument("--max-scratch", type=int, default=0)
    ap.add_argument("--max-lds", type=int, default=80 * 1024)
    a = ap.parse_args(argv)
    with open(a.asm) as f:
        status, msg = check(f.read(), a.kernel, a.max_regs, a.max_scratch, a.max_lds)
    print(msg)
    return status


if __name__ == "__main__":
    sys.exit(main())
