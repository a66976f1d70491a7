#!/usr/bin/env python3
"""Time the fused polarised calls against the compositions they replace, on the same build and in one process:
pj.sample_pol against pj.sample on the three planes plus the torch combine (and pj.sample alone on one, two and three planes),
pj.scatter_pol and pj.scatter_pol_weights against pj.scatter of the materialised (3, N) and (6, N) products, forming the
products included.  Benchmark config 5's map geometry with three components (43200 x 21601 x 3; --nx picks a smaller one if
it does not fit), points from fill_sphere_points_ (seed 42), responses and values from fill_random_.

    python tools/time_pol.py [--points 100000000] [--orders 1,3] [--rounds 1] [--burst 3] [--step-limit 120] [--out profiles/pol_times.json]

Each variant is timed in bursts of one untimed launch plus `burst` launches between hipEvents (as tools/time_scatter.py does),
the variants interleaved over `rounds`.  Every burst runs under a time limit of its own: a watchdog ends the process, with a
traceback, if one takes longer than --step-limit seconds.  Order 3 is timed on coefficients (prefiltered=True): the kernels,
not the prefilter both sides share.  Prints one JSON line: median, min and max ms per launch and, per pair, composition /
fused.  Not a test and not the benchmark: no threshold."""
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
    ap.add_argument("--orders", default="1,3")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--burst", type=int, default=3, help="timed launches per variant and round, behind one untimed launch")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds one burst may take before the process is ended")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    orders = [int(o) for o in args.orders.split(",")]
    assert args.burst >= 3 and args.rounds >= 1 and set(orders) <= {1, 3}
    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda:0")
    shape, wcs = pj.fullsky_geometry(2 * math.pi / args.nx)
    nx, ny = shape
    n = args.points
    sky = torch.empty((n, 2), dtype=torch.float64, device=dev)
    pj.fill_sphere_points_(sky, 42)
    resp = torch.empty((n, 2), dtype=torch.float64, device=dev)
    pj.fill_random_(resp, 43)
    vals = torch.empty((n,), dtype=torch.float64, device=dev)
    pj.fill_random_(vals, 44)
    q, u = resp[:, 0], resp[:, 1]
    maps = torch.empty((6, ny, nx), dtype=torch.float64, device=dev)       # planes 0..2 are the IQU map of the forward calls
    pj.fill_random_(maps, 45)
    m3 = pj.Enmap(maps[:3], wcs)
    torch.cuda.synchronize()

    def compose_sample(order):
        s = pj.sample(m3, sky, order=order, prefiltered=order == 3)
        return (s[0] + q * s[1]) + u * s[2]

    def compose_scatter(order, mode):
        t1, t2 = q * vals, u * vals
        t = [vals, t1, t2] + ([q * t1, q * t2, u * t2] if mode else [])
        return pj.scatter(torch.stack(t), sky, shape, wcs, order=order, out=maps[:len(t)], prefiltered=order == 3)

    variants = {}
    for o in orders:
        pre = {"order": o, "prefiltered": o == 3}
        variants["sample_pol_o%d" % o] = lambda pre=pre: pj.sample_pol(m3, sky, resp, **pre)
        variants["sample_compose_o%d" % o] = lambda o=o: compose_sample(o)
        for nc in (1, 2, 3):
            variants["sample_%dplane_o%d" % (nc, o)] = lambda nc=nc, pre=pre: pj.sample(pj.Enmap(maps[:nc], wcs), sky, **pre)
        variants["scatter_pol_o%d" % o] = lambda pre=pre: pj.scatter_pol(vals, sky, resp, shape, wcs, out=maps[:3], **pre)
        variants["scatter_compose_o%d" % o] = lambda o=o: compose_scatter(o, 0)
        variants["weights_pol_o%d" % o] = lambda pre=pre: pj.scatter_pol_weights(vals, sky, resp, shape, wcs, out=maps, **pre)
        variants["weights_compose_o%d" % o] = lambda o=o: compose_scatter(o, 1)
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, run in variants.items():
            faulthandler.dump_traceback_later(args.step_limit, exit=True)      # this burst's own time limit
            run()                                            # untimed: the burst's timed launches follow a launch of their own kind
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
    for o in orders:
        for pair in ("sample", "scatter", "weights"):
            fused = rec["%s_pol_o%d" % (pair, o)]["median_ms"]
            rec["%s_compose_over_fused_o%d" % (pair, o)] = round(rec["%s_compose_o%d" % (pair, o)]["median_ms"] / fused, 3)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
