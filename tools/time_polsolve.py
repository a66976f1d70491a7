#!/usr/bin/env python3
"""Time the per-pixel IQU block solve in place, with and without the rcond plane, on full-sky maps of
43200 x 21601 and 21600 x 10801 pixels, and at the smaller size what a user does without it: stack the six planes to
(npix, 3, 3) and call torch.linalg.solve, in chunks of --compose-chunk blocks (one call on the whole map fails to allocate inside hipBLAS).  Every
block is well conditioned (diagonal 3 + U(0, 1), off-diagonal U(0, 0.5)), so torch's solve neither raises nor returns garbage
and the kernel masks nothing.

    python tools/time_polsolve.py [--sizes 43200,21600] [--compose-size 21600] [--compose-chunk 4194304] [--rounds 1] [--burst 3] [--step-limit 120]
                                  [--out profiles/polsolve_times.json]

Each variant is timed in bursts of one untimed launch plus `burst` launches between hipEvents (as tools/time_pol.py does).
Every burst runs under a time limit of its own: a watchdog ends the process, with a traceback, if one takes longer than
--step-limit seconds.  The kernel reads 96 B and writes 24 B per pixel (32 B with the rcond plane): GB/s of those 120 B or
128 B is reported against the 8 TB/s of the data sheet and the 6.29 TB/s copy ceiling measured on this chip
(profiles/r01_copy_ceiling.txt).  Prints one JSON line.  Not a test and not the benchmark: no threshold."""
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

PEAK_TBS, COPY_TBS = 8.0, 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="43200,21600", help="columns of the full-sky maps (rows = nx / 2 + 1)")
    ap.add_argument("--compose-size", type=int, default=21600, help="the size at which stack + torch.linalg.solve is timed too (0: skip)")
    ap.add_argument("--compose-chunk", type=int, default=1 << 22, help="blocks per torch.linalg.solve call")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--burst", type=int, default=3, help="timed launches per variant and round, behind one untimed launch")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds one burst may take before the process is ended")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    assert args.burst >= 3 and args.rounds >= 1
    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda:0")
    rec = {"rounds": args.rounds, "burst": args.burst, "device": torch.cuda.get_device_name(dev), "peak_tbs": PEAK_TBS, "copy_ceiling_tbs": COPY_TBS}

    def burst(name, run, times):
        faulthandler.dump_traceback_later(args.step_limit, exit=True)          # this burst's own time limit
        run()                                                # untimed: the burst's timed launches follow a launch of their own kind
        for _b in range(args.burst):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times.setdefault(name, []).append(e0.elapsed_time(e1))
        faulthandler.cancel_dump_traceback_later()
        print("%s: %s ms" % (name, ", ".join("%.2f" % t for t in times[name][-args.burst:])), file=sys.stderr, flush=True)

    for nx in sizes:
        shape, wcs = pj.fullsky_geometry(2 * math.pi / nx)
        nx, ny = shape
        npix = nx * ny
        w = torch.empty((6, ny, nx), dtype=torch.float64, device=dev)
        pj.fill_random_(w, 45, kind="uniform")
        w[1:3] *= 0.5
        w[4] *= 0.5
        for c in (0, 3, 5):
            w[c] += 3.0
        r = torch.empty((3, ny, nx), dtype=torch.float64, device=dev)
        pj.fill_random_(r, 46)
        keep = r.clone()
        wts, rhs = pj.Enmap(w, wcs), pj.Enmap(r, wcs)
        torch.cuda.synchronize()
        variants = {"solve_inplace": lambda: pj.pol_block_solve(rhs, wts, out=rhs),
                    "solve_inplace_rcond": lambda: pj.pol_block_solve(rhs, wts, out=rhs, return_rcond=True)}
        if nx == args.compose_size:
            xs = torch.empty((npix, 3), dtype=torch.float64, device=dev)

            def compose():
                # in chunks: one call on all 2.3e8 blocks of the 21600 x 10801 map fails inside hipBLAS (HIPBLAS_STATUS_ALLOC_FAILED)
                for lo in range(0, npix, args.compose_chunk):
                    a, b, c, d, e, f = w.view(6, -1)[:, lo:lo + args.compose_chunk]
                    A = torch.stack([a, b, c, b, d, e, c, e, f], dim=1).view(-1, 3, 3)
                    xs[lo:lo + args.compose_chunk] = torch.linalg.solve(A, r.view(3, -1)[:, lo:lo + args.compose_chunk].t().unsqueeze(-1))[:, :, 0]
                return xs
            variants["stack_linalg_solve"] = compose
        times = {}
        for _ in range(args.rounds):
            for name, run in variants.items():
                r.copy_(keep)                                # the in-place solves start from the same right-hand side every burst
                burst(name, run, times)
        size = {"map": [nx, ny], "npix": npix}
        for name, t in times.items():
            t = sorted(t)
            size[name] = {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}
        for name, nbytes in (("solve_inplace", 120), ("solve_inplace_rcond", 128)):
            gbs = npix * nbytes / (size[name]["median_ms"] * 1e-3) / 1e9
            size[name].update(bytes_per_pixel=nbytes, gb_per_s=round(gbs, 1), of_peak=round(gbs / (PEAK_TBS * 1e3), 3),
                              of_copy_ceiling=round(gbs / (COPY_TBS * 1e3), 3))
        if "stack_linalg_solve" in size:
            size["stack_linalg_solve"]["chunk_blocks"] = args.compose_chunk
            size["stack_linalg_solve_over_kernel"] = round(size["stack_linalg_solve"]["median_ms"] / size["solve_inplace"]["median_ms"], 2)
        rec["nx_%d" % nx] = size
        if args.out:
            with open(args.out, "w") as f:                   # after every size: a later burst's time limit loses nothing measured
                f.write(json.dumps(rec) + "\n")
        del w, r, keep, wts, rhs, variants
        xs = None
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
