#!/usr/bin/env python3
"""Time the two passes of the destriper, pj.baseline_bin_pol_nearest and pj.baseline_project_pol_nearest, against
the torch composition they replace, and one full application of the destriping operator, on the same build and in one process.
Benchmark config 5's map geometry with three components (43200 x 21601 x 3; --nx picks a smaller one if it does not fit) and one
chunk of --dets x --samples samples (1000 x 10^5), for baseline_len 100 and 10^4, on two workloads:

    sphere   points from fill_sphere_points_ (seed 42): every sample lands in a pixel of its own, no locality;
    raster   samples in scan order: half a pixel apart along a row, the row sweeps half a pixel apart, in a band about the
             equator, detector after detector -- as scan-ordered time streams are.

What is timed, per workload and baseline length, with a = p as in an application of the operator:

    bin          baseline_bin_pol_nearest(a=p, mask) into a map
    project      baseline_project_pol_nearest(a=p, m, mask) into the baselines
    compose_bin      Fa = repeat_interleave(p), scatter_pol_nearest(wm * Fa)                    (wm: w with the mask applied, made once)
    compose_project  Fa likewise, s = sample_pol_nearest(m), (wm * (Fa - s)) padded, reshaped to (D, n_base, len) and summed
    apply        one full A p: bin into a zeroed map, pol_block_solve against the weights, project

    python tools/time_destripe.py [--dets 1000] [--samples 100000] [--rounds 1] [--burst 3] [--step-limit 120] [--out profiles/destripe_times.json]

Each variant is timed in bursts of one untimed call plus `burst` calls between hipEvents (as tools/time_nearest.py does), the
variants interleaved over `rounds`.  Every burst runs under a time limit of its own: a watchdog ends the process, with a traceback,
if one takes longer than --step-limit seconds; nothing is retried.  Prints one JSON line: median, min and max ms per call and the
ratios composition / fused.  Not a test and not the benchmark: no threshold."""
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
    ap.add_argument("--dets", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=10 ** 5, help="time samples per detector")
    ap.add_argument("--nx", type=int, default=43200, help="columns of the full-sky map (rows = nx / 2 + 1)")
    ap.add_argument("--lens", type=int, nargs="+", default=[100, 10 ** 4], help="baseline lengths")
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
    nd, nt = args.dets, args.samples
    n = nd * nt
    f64 = dict(dtype=torch.float64, device=dev)
    rhs = pj.Enmap(torch.zeros((3, ny, nx), **f64), wcs)
    m = pj.Enmap(torch.empty((3, ny, nx), **f64), wcs)
    pj.fill_random_(m.data.view(-1), 46)
    mask = torch.ones((ny, nx), **f64)
    mask[::7, ::5] = 0.0                                                  # one pixel in 35 masked
    resp = torch.empty((n, 2), **f64)
    pj.fill_random_(resp, 43)
    w = torch.empty((n,), **f64)
    pj.fill_random_(w, 44, kind="uniform")
    skies = {"sphere": torch.empty((n, 2), **f64), "raster": torch.empty((n, 2), **f64)}
    pj.fill_sphere_points_(skies["sphere"], 42)
    k = torch.arange(n, **f64)
    sweep = torch.floor(k / (2 * nx))                                   # 2 nx points per row sweep
    pix = skies["raster"]
    pix[:, 0] = 1.0 + 0.5 * (k - sweep * (2 * nx))
    pix[:, 1] = max(1.0, ny / 2.0 - 0.25 * n / (2 * nx)) + 0.5 * sweep
    assert float(pix[:, 1].max()) < ny, "the raster band does not fit the map: fewer samples, or a larger --nx"
    del k, sweep
    pj.pix2sky_(rhs, pix, pix, safe=False)
    wm = {name: w * (pj.sample_nearest(pj.Enmap(mask, wcs), sky)[0] > 0) for name, sky in skies.items()}    # the composition's masked weights
    weights = pj.Enmap(torch.zeros((6, ny, nx), **f64), wcs)
    torch.cuda.synchronize()

    variants = {}
    for blen in args.lens:
        nb = -(-nt // blen)
        p = torch.empty((nd * nb,), **f64)
        pj.fill_random_(p, 47)
        outb = torch.zeros((nd * nb,), **f64)
        lay = (shape, wcs, nd, 0, blen, nb)

        def spread(p=p, blen=blen, nb=nb):
            return torch.repeat_interleave(p.view(nd, nb), blen, dim=1)[:, :nt].reshape(-1)

        def compose_bin(sky, name, spread=spread):
            pj.scatter_pol_nearest(wm[name] * spread(), sky, resp, shape, wcs, out=rhs)

        def compose_project(sky, name, spread=spread, blen=blen, nb=nb, outb=outb, src=m):
            t = wm[name] * (spread() - pj.sample_pol_nearest(src, sky, resp))
            t = torch.nn.functional.pad(t.view(nd, nt), (0, nb * blen - nt))
            outb.add_(t.view(nd, nb, blen).sum(-1).reshape(-1))

        def apply(sky, p=p, lay=lay, outb=outb):
            rhs.data.zero_()
            pj.baseline_bin_pol_nearest(w, sky, resp, *lay, a=p, mask=mask, out=rhs)
            pj.pol_block_solve(rhs, weights, out=rhs)
            pj.baseline_project_pol_nearest(w, sky, resp, *lay, a=p, m=rhs, mask=mask, out=outb)

        for name, sky in skies.items():
            tag = "_%s_len%d" % (name, blen)
            variants["bin" + tag] = lambda sky=sky, p=p, lay=lay: pj.baseline_bin_pol_nearest(w, sky, resp, *lay, a=p, mask=mask, out=rhs)
            variants["project" + tag] = lambda sky=sky, p=p, lay=lay, outb=outb: pj.baseline_project_pol_nearest(w, sky, resp, *lay, a=p, m=m, mask=mask, out=outb)
            variants["compose_bin" + tag] = lambda sky=sky, name=name, f=compose_bin: f(sky, name)
            variants["compose_project" + tag] = lambda sky=sky, name=name, f=compose_project: f(sky, name)
            variants["apply" + tag] = lambda sky=sky, f=apply: f(sky)
    for sky in skies.values():                                          # one weight map of both pointings serves every apply: the solve
        pj.scatter_pol_weights_nearest(w, sky, resp, shape, wcs, out=weights)    # visits every pixel whichever are solved
    torch.cuda.synchronize()
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
    rec = {"map": [nx, ny, 3], "dets": nd, "samples": nt, "rounds": args.rounds, "burst": args.burst, "device": torch.cuda.get_device_name(dev)}
    for name, t in times.items():
        t = sorted(t)
        rec[name] = {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}
    for blen in args.lens:
        for name in skies:
            tag = "_%s_len%d" % (name, blen)
            for kind in ("bin", "project"):
                rec["compose_over_fused_%s%s" % (kind, tag)] = round(rec["compose_" + kind + tag]["median_ms"] / rec[kind + tag]["median_ms"], 3)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
