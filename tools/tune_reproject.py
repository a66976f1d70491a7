#!/usr/bin/env python3
"""Interleaved A/B timing of reprojection launch configurations (one process, N variants x M
rounds, median and min reported -- cdna_hip_programming.md rule 24).

    python tools/tune_reproject.py --workload cfg4 --rounds 7 "rh=64,pairs=2" "rh=16,pairs=1" "rh=16,nt=0"

Variant keys map to the PXL_REPROJECT_* environment knobs read at plan creation.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import pixell_jl_amd as pj  # noqa: E402

KEYS = {"rh": "PXL_REPROJECT_RH", "pairs": "PXL_REPROJECT_PAIRS", "pf": "PXL_REPROJECT_PF", "ns": "PXL_REPROJECT_NS",
        "nt": "PXL_REPROJECT_NT"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg4")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--burst", type=int, default=3, help="timed launches per variant and round, behind one untimed launch of the same variant")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--placements", type=int, default=1, help="re-allocate the maps this many times (physical placement moves the kernel by up to 10 %%) and print every variant per placement")
    ap.add_argument("--place", action="store_true", help="maps from pj.place_pair (destination across a boundary between two memory classes) instead of torch.empty")
    ap.add_argument("--place-native", action="store_true", help="maps from the C ABI's pxl_mem_pair_alloc (pj.place_pair_native)")
    ap.add_argument("--place-compact", action="store_true", help="maps from pj.place_pair_compact (two-class destination without head-room)")
    ap.add_argument("--strip", default=None, help="R/W: time the declination strip of rank R of W (interior rows only)")
    ap.add_argument("variants", nargs="+")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    shape_in, wcs_in, shape_out, wcs_out, desc = bench.workload_geometry(args.workload)
    nx, ny, nc = shape_in
    nxo, nyo = shape_out
    src_rows = dst_rows = None
    r0, nr = 0, nyo
    if args.strip:
        rank, world = (int(v) for v in args.strip.split("/"))
        lay = pj.DecStripLayout(shape_in, wcs_in, shape_out, wcs_out, rank, world)
        src_rows, dst_rows = lay.src_window, lay.dst_window
        r0, nr = lay.interior[0], lay.interior[1] - lay.interior[0]
        desc += "  [strip %d/%d: %d source rows, %d interior output rows]" % (rank, world, src_rows[1], nr)
    ny_s = src_rows[1] if src_rows else ny
    nyo_s = dst_rows[1] if dst_rows else nyo
    if args.dtype == "f32":
        src = torch.randn((nc, ny_s, nx), dtype=torch.float32, device=dev)
        dst = torch.empty((nc, nyo_s, nxo), dtype=torch.float32, device=dev)
    elif args.place_compact:
        import time
        t0 = time.perf_counter()
        src, dst, info = pj.place_pair_compact((nc, ny_s, nx), (nc, nyo_s, nxo), dtype=torch.float64, device=dev)
        print("place_pair_compact: %.2f s" % (time.perf_counter() - t0), info, "allocated now: %.1f GiB" % (torch.cuda.memory_reserved(dev) / 2**30))
        pj.fill_random_(src, 1234)
    elif args.place_native:
        import time
        t0 = time.perf_counter()
        src, dst, info = pj.place_pair_native((nc, ny_s, nx), (nc, nyo_s, nxo), dtype=torch.float64, device=dev)
        arena_keep = info.pop("owner")
        print("place_pair_native: %.2f s" % (time.perf_counter() - t0), info)
        pj.fill_random_(src, 1234)
    elif args.place:
        import time
        t0 = time.perf_counter()
        src, dst, info = pj.place_pair((nc, ny_s, nx), (nc, nyo_s, nxo), dtype=torch.float64, device=dev)
        arena_keep = info.pop("arena")
        print("place_pair: %.2f s" % (time.perf_counter() - t0), info)
        pj.fill_random_(src, 1234)
    else:
        src = torch.empty((nc, ny_s, nx), dtype=torch.float64, device=dev)
        dst = torch.empty((nc, nyo_s, nxo), dtype=torch.float64, device=dev)
        pj.fill_random_(src, 1234)
    plans = []
    for v in args.variants:
        for k in KEYS.values():
            os.environ.pop(k, None)
        for kv in v.split(","):
            if kv:
                k, val = kv.split("=")
                os.environ[KEYS[k]] = val
        plans.append(pj.ReprojectPlan(shape_in, wcs_in, shape_out, wcs_out, src_rows=src_rows, dst_rows=dst_rows, device=dev))
    import random
    alg = (4.0 if args.dtype == "f32" else 8.0) * nc * (nx * ny_s + nxo * nr)
    print("workload:", desc)
    keep = []
    for place in range(args.placements):
        if place > 0:                                # move the maps: free, perturb the heap, allocate again
            tdt = src.dtype
            del src, dst
            keep.append(torch.empty(int(random.uniform(0.3, 3.0) * 2**30), dtype=torch.uint8, device=dev))
            keep = keep[-2:]
            torch.cuda.empty_cache()
            src = torch.randn((nc, ny_s, nx), dtype=tdt, device=dev) if tdt == torch.float32 else torch.empty((nc, ny_s, nx), dtype=tdt, device=dev)
            if tdt == torch.float64:
                pj.fill_random_(src, 1234)
            dst = torch.empty((nc, nyo_s, nxo), dtype=tdt, device=dev)
        for pl in plans:
            pl.build_tables()
            pl.execute_rows(src, dst, r0, nr)       # warm-up
        torch.cuda.synchronize()
        times = [[] for _ in plans]
        for _ in range(args.rounds):
            for i, pl in enumerate(plans):
                # a BURST per variant: what a launch leaves in the L2 / Infinity Cache (dirty lines of plain stores, nothing after
                # non-temporal ones) changes the NEXT launch by 2 % on multi-GB maps and by up to 20 % on a 1/8 strip (round 4:
                # one launch per variant, interleaved, timed each variant behind ANOTHER variant's launch).  The first launch of
                # the burst is not timed; the others are what a caller repeating one plan sees (bench.py's steady state)
                pl.execute_rows(src, dst, r0, nr)
                for _b in range(args.burst):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    pl.execute_rows(src, dst, r0, nr)
                    e1.record()
                    torch.cuda.synchronize()
                    times[i].append(e0.elapsed_time(e1))
        if args.placements > 1:
            print("-- placement %d" % place)
        for v, t in zip(args.variants, times):
            t = sorted(t)
            med, mn = t[len(t) // 2], t[0]
            print("%-40s median %8.4f ms  min %8.4f ms  -> %7.1f GB/s (%.1f%% of 8 TB/s)" % (
                v, med, mn, alg / med / 1e6, alg / med / 1e6 / 80.0))


if __name__ == "__main__":
    main()
