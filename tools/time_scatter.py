#!/usr/bin/env python3
"""Time pj.scatter_bilinear (FP64 atomic scatter-add) and pj.scatter_cubic (its order-3 counterpart, sixteen
taps per point) next to the forward pj.sample_bilinear on benchmark config 5's map geometry (43200 x 21601,
one component), in one process.

    python tools/time_scatter.py [--points 100000000] [--rounds 3] [--burst 3] [--out profiles/scatter_times.json]

Two orders of the same fill_sphere_points_ (seed 42) points: as generated (random), and sorted by (row, column) of their
cell -- a scan-like stream in which neighbouring lanes add into the same pixels.  Each variant is timed in bursts of one
untimed launch plus `burst` launches between hipEvents (as tools/tune_reproject.py does), the variants interleaved over
`rounds`.  Prints one JSON line: median and min ms per launch, ms per 1e8 points, and for the scatter the atomic bytes per
second they imply (4 taps x 8 bytes per point and component, 16 x 8 for order 3), and the order-3 / order-1 ratio of the
scatter medians.  Not a test and not the benchmark: no threshold."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import pixell_jl_amd as pj  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10 ** 8)
    ap.add_argument("--nx", type=int, default=43200, help="columns of the full-sky map (rows = nx / 2 + 1)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--burst", type=int, default=3, help="timed launches per variant and round, behind one untimed launch")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    assert args.burst >= 3 and args.rounds >= 1
    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda:0")
    shape, wcs = pj.fullsky_geometry(2 * math.pi / args.nx)
    nx, ny = shape
    n = args.points
    sky = torch.empty((n, 2), dtype=torch.float64, device=dev)
    pj.fill_sphere_points_(sky, 42)
    vals = torch.empty((1, n), dtype=torch.float64, device=dev)
    pj.fill_random_(vals, 43)
    # the same points sorted by (row, column) of their cell
    pix = pj.sky2pix((shape, wcs), sky, safe=True)
    key = torch.floor(pix[:, 1]).to(torch.int64) * (nx + 2) + torch.floor(pix[:, 0]).to(torch.int64)
    del pix
    perm = torch.argsort(key)
    del key
    sky_s = sky[perm].contiguous()
    vals_s = vals[:, perm].contiguous()
    del perm
    m = pj.Enmap(torch.zeros((1, ny, nx), dtype=torch.float64, device=dev), wcs)       # (nc, ny, nx): what (nc, N) values accumulate into
    torch.cuda.synchronize()

    variants = {
        "scatter_random": lambda: pj.scatter_bilinear(vals, sky, shape, wcs, out=m),
        "scatter_sorted": lambda: pj.scatter_bilinear(vals_s, sky_s, shape, wcs, out=m),
        "scatter_cubic_random": lambda: pj.scatter_cubic(vals, sky, shape, wcs, out=m),
        "scatter_cubic_sorted": lambda: pj.scatter_cubic(vals_s, sky_s, shape, wcs, out=m),
        "sample_random": lambda: pj.sample_bilinear(m, sky),
        "sample_sorted": lambda: pj.sample_bilinear(m, sky_s),
    }
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, run in variants.items():
            run()                                            # untimed: the burst's timed launches follow a launch of their own kind
            for _b in range(args.burst):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
    rec = {"map": [nx, ny, 1], "points": n, "rounds": args.rounds, "burst": args.burst, "device": torch.cuda.get_device_name(dev)}
    for name, t in times.items():
        t = sorted(t)
        med, mn = t[len(t) // 2], t[0]
        r = {"median_ms": round(med, 3), "min_ms": round(mn, 3), "max_ms": round(t[-1], 3), "ms_per_1e8_points": round(med * 1e8 / n, 3)}
        if name.startswith("scatter"):
            r["atomic_GB_per_s"] = round((16 if "cubic" in name else 4) * 8 * n / med / 1e6, 1)
        rec[name] = r
    for order in ("random", "sorted"):
        rec["cubic_over_bilinear_" + order] = round(rec["scatter_cubic_" + order]["median_ms"] / rec["scatter_" + order]["median_ms"], 3)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
