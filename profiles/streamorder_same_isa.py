#!/usr/bin/env python3
"""The gfx950 device code of every .hip unit, parent tree against changed tree: compiled with the flags cubicsdr_amd/build.py
uses, device side only, to assembly; compared per unit as text (all of it: instructions, kernel descriptors, metadata; only the lines
of the __hip_cuid_ symbol are left out), and per symbol where a unit differs.

    python profiles/streamorder_same_isa.py PARENT_TREE CHANGED_TREE > profiles/streamorder_same_isa.txt
"""
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


def device_asm(tree, unit, out):
    src = os.path.join(tree, "cubicsdr_amd", "csrc", unit)
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "--cuda-device-only", "-S", src, "-o", out], check=True, cwd=tree)
    with open(out) as f:        # (__hip_cuid_<hash> is the unit's id, hashed from its path and text: no code)
        return "".join(line for line in f if "__hip_cuid_" not in line)


def by_symbol(asm):
    """symbol -> its lines: a symbol starts at a label in column 0 and ends at the next one"""
    syms, cur = {}, "(header)"
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1)
        syms.setdefault(cur, []).append(line)
    return syms


def main():
    parent, changed = sys.argv[1], sys.argv[2]
    units = sorted(os.path.basename(p) for p in glob.glob(os.path.join(changed, "cubicsdr_amd", "csrc", "*.hip")))
    print("flags: hipcc %s --cuda-device-only -S" % " ".join(FLAGS))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as pool:
        jobs = {u: (pool.submit(device_asm, parent, u, os.path.join(tmp, "p_" + u + ".s")),
                    pool.submit(device_asm, changed, u, os.path.join(tmp, "c_" + u + ".s"))) for u in units}
        for u in units:
            a, b = jobs[u][0].result(), jobs[u][1].result()
            n_kernels = len(re.findall(r"^\s*\.amdhsa_kernel ", b, re.M))
            if a == b:
                print("%-22s equal  (%d kernels, %d lines of assembly)" % (u, n_kernels, b.count("\n")))
                continue
            sa, sb = by_symbol(a), by_symbol(b)
            diff = sorted(s for s in set(sa) | set(sb) if sa.get(s) != sb.get(s))
            print("%-22s DIFFERS in: %s" % (u, ", ".join(diff)))


if __name__ == "__main__":
    main()
