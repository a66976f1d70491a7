"""Time distance_transform (pxl_distance_transform_car_f64) on the 43200 x 21601 CC map (0.5 arcmin) with three seeded masks:
about 2000 disks of 5 arcmin radius (a point-source mask), the band |DEC| < 10 degrees, and a single zero pixel.
hipEvent timing (torch.cuda.Event), median of --reps launches after 3 warm-ups; the effective rate counts 16 B per pixel
(the map read, the distances written) against 8 TB/s.  Prints one JSON line per mask."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pixell_jl_amd as pj  # noqa: E402
import sdt_ref as R  # noqa: E402

PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res-arcmin", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pj.load_library()
    shape, wcs = pj.fullsky_geometry(a.res_arcmin * math.pi / 180 / 60)
    nx, ny = shape
    out = torch.empty((ny, nx), dtype=torch.float64, device=dev)
    m = torch.ones((ny, nx), dtype=torch.float64, device=dev)
    lib = pj.load_library()
    st = torch.cuda.current_stream(dev)
    for mask in ("sources", "band", "single"):
        m.fill_(1.0)
        if mask == "sources":
            zi, zj = R.disk_zeros(wcs, shape, 2000, 5 * math.pi / 180 / 60, seed=7)
            m.view(-1)[torch.from_numpy(zj * nx + zi).to(dev)] = 0.0
        elif mask == "band":
            m[torch.from_numpy(R.band_rows(wcs, shape, 10 * math.pi / 180)).to(dev)] = 0.0
        else:
            rng = np.random.default_rng(5)
            m[int(rng.integers(0, ny)), int(rng.integers(0, nx))] = 0.0
        nzero = int((m == 0).sum().item())
        em = pj.Enmap(m, wcs)
        times = []
        for r in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            pj._lib.check(lib.pxl_distance_transform_car_f64(pj.ops._wcs_ref(wcs), pj.ops._shape2(shape), pj.ops._ptr(m),
                                                             pj.ops._ptr(out), pj.ops._stream(m)))
            e1.record(st)
            e1.synchronize()
            if r >= a.warmup:
                times.append(e0.elapsed_time(e1))
        pj.distance_transform(pj.ExactSeqSDT(), em, out=pj.Enmap(out, wcs))     # the public path once (raises on no zero)
        ms = float(np.median(times))
        rate = 16.0 * nx * ny / (ms * 1e-3)
        print(json.dumps({"mask": mask, "shape": [nx, ny], "zeros": nzero, "median_ms": round(ms, 3),
                          "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "reps": a.reps,
                          "eff_TBps": round(rate / 1e12, 3), "frac_of_8TBps": round(rate / PEAK, 4)}), flush=True)


if __name__ == "__main__":
    main()
