"""Time the cubic B-spline path beside the bilinear one on the BASELINE.md config 2 ((4096, 2049) -> (8192, 4097)) and
config 3 ((21600, 10801) -> (43200, 21601)) geometries: bilinear pj.reproject, pj.reproject(order=3) with and without
prefiltered=True, and pj.spline_prefilter alone.  hipEvent timing (torch.cuda.Event), median of --reps launches after
--warmup warm-ups, outputs and plan allocated once.  Algorithmic bytes: 16 B per source pixel per prefilter axis pass (two
passes), 8 (N_src + N_dst) for an evaluation, as for bilinear.  Prints one JSON line."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pixell_jl_amd as pj  # noqa: E402


def timed(fn, st, warmup, reps):
    times = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        if r >= warmup:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert a.reps >= 1
    dev = torch.device("cuda:0")
    pj.load_library()
    st = torch.cuda.current_stream(dev)
    result = {"reps": a.reps, "warmup": a.warmup, "configs": {}}
    for cfg in [int(c) for c in a.configs.split(",")]:
        nx = {2: 4096, 3: 21600}[cfg]
        shape_in, wcs_in = pj.fullsky_geometry(2 * math.pi / nx)
        shape_out, wcs_out = pj.fullsky_geometry(2 * math.pi / (2 * nx))
        nsrc, ndst = shape_in[0] * shape_in[1], shape_out[0] * shape_out[1]
        src = torch.empty((shape_in[1], shape_in[0]), dtype=torch.float64, device=dev)
        pj.fill_random_(src, 1234)
        m = pj.Enmap(src, wcs_in)
        coeffs = pj.Enmap(torch.empty_like(src), wcs_in)
        out = pj.Enmap(torch.empty((shape_out[1], shape_out[0]), dtype=torch.float64, device=dev), wcs_out)
        plan = pj.ReprojectPlan(shape_in, wcs_in, shape_out, wcs_out, device=dev)
        pj.spline_prefilter(m, out=coeffs)
        legs = {
            "bilinear": (lambda: pj.reproject(m, shape_out, wcs_out, out=out, plan=plan), 8.0 * (nsrc + ndst)),
            "prefilter": (lambda: pj.spline_prefilter(m, out=coeffs), 32.0 * nsrc),
            "cubic_prefiltered": (lambda: pj.reproject(coeffs, shape_out, wcs_out, out=out, order=3, prefiltered=True), 8.0 * (nsrc + ndst)),
            "cubic_one_call": (lambda: pj.reproject(m, shape_out, wcs_out, out=out, order=3), 32.0 * nsrc + 8.0 * (nsrc + ndst)),
        }
        rec = {"shape_in": list(shape_in), "shape_out": list(shape_out)}
        for name, (fn, nbytes) in legs.items():
            med, lo, hi = timed(fn, st, a.warmup, a.reps)
            npix = nsrc if name == "prefilter" else ndst
            rec[name] = {"median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                         "Mpix_per_s": round(npix / med / 1e3, 1), "algorithmic_GBps": round(nbytes / med / 1e6, 1)}
        rec["cubic_prefiltered_over_bilinear"] = round(rec["cubic_prefiltered"]["median_ms"] / rec["bilinear"]["median_ms"], 3)
        rec["cubic_one_call_over_bilinear"] = round(rec["cubic_one_call"]["median_ms"] / rec["bilinear"]["median_ms"], 3)
        result["configs"]["cfg%d" % cfg] = rec
        del src, coeffs, out, plan, m
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
