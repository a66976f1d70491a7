#!/usr/bin/env python3
"""Time the fused map-making pass of nearest-pixel pointing, pj.bin_pol_nearest, against the composition it
replaces, scatter_pol_nearest(w * d) + scatter_pol_weights_nearest(w), and against the order-1 accumulation
scatter_pol(w * d) + scatter_pol_weights(w) for scale, on the same build and in one process.  Benchmark config 5's map geometry with
three components (43200 x 21601 x 3, and six weight planes beside it; --nx picks a smaller one if it does not fit), two workloads
of --points points each:

    sphere   points from fill_sphere_points_ (seed 42): every point lands in a pixel of its own, no locality;
    raster   points in scan order: half a pixel apart along a row, the row sweeps half a pixel apart, in a band about the
             equator -- consecutive lanes hit the same or neighbouring pixels, as scan-ordered time streams do.

    python tools/time_nearest.py [--points 100000000] [--rounds 1] [--burst 3] [--step-limit 120] [--out profiles/nearest_times.json]

Each variant is timed in bursts of one untimed call plus `burst` calls between hipEvents (as tools/time_normal.py does), the
variants interleaved over `rounds`.  Every burst runs under a time limit of its own: a watchdog ends the process, with a
traceback, if one takes longer than --step-limit seconds; nothing is retried.  The composition's two scatters are also timed alone.
Prints one JSON line: median, min and max ms per call and, per workload, composition / fused and order 1 / fused.  Not a test and
not the benchmark: no threshold."""
import argparse
import faulthandler
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
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--burst", type=int, default=3, help="timed calls per variant and round, behind one untimed call")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds one burst may take before the process is ended")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    assert args.burst >= 3 and args.rounds >= 1
    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda:0")
    shape, wcs = pj.fullsky_geometry(2 * math.pi / args.nx)
    nx, ny = shape
    n = args.points
    rhs = pj.Enmap(torch.zeros((3, ny, nx), dtype=torch.float64, device=dev), wcs)
    wts = pj.Enmap(torch.zeros((6, ny, nx), dtype=torch.float64, device=dev), wcs)
    resp = torch.empty((n, 2), dtype=torch.float64, device=dev)
    pj.fill_random_(resp, 43)
    w = torch.empty((n,), dtype=torch.float64, device=dev)
    pj.fill_random_(w, 44, kind="uniform")
    d = torch.empty((n,), dtype=torch.float64, device=dev)
    pj.fill_random_(d, 45)
    skies = {"sphere": torch.empty((n, 2), dtype=torch.float64, device=dev), "raster": torch.empty((n, 2), dtype=torch.float64, device=dev)}
    pj.fill_sphere_points_(skies["sphere"], 42)
    k = torch.arange(n, dtype=torch.float64, device=dev)
    sweep = torch.floor(k / (2 * nx))                                   # 2 nx points per row sweep
    pix = skies["raster"]
    pix[:, 0] = 1.0 + 0.5 * (k - sweep * (2 * nx))
    pix[:, 1] = max(1.0, ny / 2.0 - 0.25 * n / (2 * nx)) + 0.5 * sweep
    assert float(pix[:, 1].max()) < ny, "the raster band does not fit the map: fewer points, or a larger --nx"
    del k, sweep
    pj.pix2sky_(rhs, pix, pix, safe=False)
    torch.cuda.synchronize()

    def compose(sky):
        pj.scatter_pol_nearest(w * d, sky, resp, shape, wcs, out=rhs)
        pj.scatter_pol_weights_nearest(w, sky, resp, shape, wcs, out=wts)

    def order1(sky):
        pj.scatter_pol(w * d, sky, resp, shape, wcs, out=rhs)
        pj.scatter_pol_weights(w, sky, resp, shape, wcs, out=wts)

    variants = {}
    for name, sky in skies.items():
        variants["bin_pol_nearest_" + name] = lambda sky=sky: pj.bin_pol_nearest(d, w, sky, resp, shape, wcs, rhs=rhs, weights=wts)
        variants["compose_" + name] = lambda sky=sky: compose(sky)
        variants["scatter_pol_nearest_" + name] = lambda sky=sky: pj.scatter_pol_nearest(d, sky, resp, shape, wcs, out=rhs)   # the two scatters alone
        variants["scatter_pol_weights_nearest_" + name] = lambda sky=sky: pj.scatter_pol_weights_nearest(w, sky, resp, shape, wcs, out=wts)
        variants["order1_" + name] = lambda sky=sky: order1(sky)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, run in variants.items():
            faulthandler.dump_traceback_later(args.step_limit, exit=True)      # this burst's own time limit
            run()                                            # untimed: the burst's timed calls follow a call of their own kind
            for _b in range(args.burst):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
            faulthandler.cancel_dump_traceback_later()
            print("%s: %s ms" % (name, ", ".join("%.2f" % t for t in times[name][-args.burst:])), file=sys.stderr, flush=True)
    rec = {"map": [nx, ny, 3], "points": n, "rounds": args.rounds, "burst": args.burst, "device": torch.cuda.get_device_name(dev)}
    for name, t in times.items():
        t = sorted(t)
        rec[name] = {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}
    for name in skies:
        fused = rec["bin_pol_nearest_" + name]["median_ms"]
        rec["compose_over_fused_" + name] = round(rec["compose_" + name]["median_ms"] / fused, 3)
        rec["order1_over_fused_" + name] = round(rec["order1_" + name]["median_ms"] / fused, 3)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
