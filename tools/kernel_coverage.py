#!/usr/bin/env python3
"""Which kernel instantiations of libpixell_hip.so do the GPU tests launch?

    rocprofv3 --kernel-trace --stats --output-format csv -d gpurun_out/cov -o cov -- python3 -m pytest tests -m gpu -q
    make -C pixell.jl_amd/csrc asm
    python tools/kernel_coverage.py gpurun_out/cov/cov_kernel_stats.csv

Compares the kernel names in the rocprofv3 statistics with the kernels in the ISA listing of the library.

Which launch shapes did a run take?  Calls and the largest grid (in workgroups) of every library kernel of a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/lp -o lp -- python3 -m pytest tests/test_gpu_launch_paths.py -m gpu -q
    python tools/kernel_coverage.py --grids /tmp/lp/lp_kernel_trace.csv > profiles/launch_paths_kernel_trace.txt"""
import csv
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def norm(s):
    return re.sub(r"\s+", "", re.sub(r"\(.*$", "", s.replace("void ", "")))


def grids(trace):
    """per library kernel (k_*): calls, the largest grid in workgroups (x, y, z), the workgroup size and every distinct grid, from
    a kernel trace"""
    seen = {}
    for r in csv.DictReader(open(trace)):
        name = re.sub(r"\(.*$", "", r["Kernel_Name"].replace("void ", "")).strip()
        if not name.startswith("k_"):
            continue
        wg = [max(1, int(r["Workgroup_Size_" + a])) for a in "XYZ"]
        g = tuple(int(r["Grid_Size_" + a]) // w for a, w in zip("XYZ", wg))
        calls, shapes, _ = seen.get(name, (0, set(), wg[0]))
        shapes.add(g)
        seen[name] = (calls + 1, shapes, wg[0])
    fmt = lambda g: "%d x %d x %d" % g if g[2] > 1 else ("%d x %d" % g[:2] if g[1] > 1 else "%d" % g[0])   # noqa: E731
    print("%6s  %-16s %5s  %-34s %s" % ("calls", "largest grid", "block", "kernel", "distinct grids (workgroups)"))
    for name in sorted(seen):
        calls, shapes, wg = seen[name]
        order = sorted(shapes, key=lambda g: -(g[0] * g[1] * g[2]))
        more = ", ".join(fmt(g) for g in order[:10]) + (" ... (%d)" % len(order) if len(order) > 10 else "")
        print("%6d  %-16s %5d  %-34s %s" % (calls, fmt(order[0]), wg, name, more))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--grids":
        return grids(sys.argv[2])
    stats = sys.argv[1]
    rows = list(csv.DictReader(open(stats)))
    calls = {norm(r["Name"]): int(r["Calls"]) for r in rows}
    txt = open(os.path.join(ROOT, "pixell.jl_amd", "csrc", "pxl_kernels.gfx950.s")).read()
    syms = sorted(set(re.findall(r"\.amdhsa_kernel (\S+)", txt)))
    dem = subprocess.run(["c++filt"] + syms, capture_output=True, text=True).stdout.splitlines()
    missing = [d for d in dem if norm(d) not in calls]
    print("%d kernels in the library, %d launched by the profiled run, %d never launched" % (len(dem), len(dem) - len(missing), len(missing)))
    for d in dem:
        print("%8s  %s" % (calls.get(norm(d), "-"), re.sub(r"\(.*$", "", d.replace("void ", ""))))
    sys.exit(1 if missing else 0)


if __name__ == "__main__":
    main()
