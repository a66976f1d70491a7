#!/usr/bin/env python3
"""Time detector pointing expansion, pj.expand_pointing, against the same definition written in torch elementwise
operations -- what a user does today to get skycoords and resp from quaternion pointing -- on the same build and in one process.
Workload: --dets detectors x --samples time samples (1000 x 10^5 = 10^8 samples by default), random unit boresights and
detectors, gamma in [0, 1].

    python tools/time_pointing.py [--dets 1000] [--samples 100000] [--rounds 1] [--burst 3] [--step-limit 120] [--out profiles/pointing_times.json]

Each variant is timed in bursts of one untimed call plus `burst` calls between hipEvents (as tools/time_nearest.py does), the
variants interleaved over `rounds`.  Every burst runs under a time limit of its own: a watchdog ends the process, with a
traceback, if one takes longer than --step-limit seconds; nothing is retried.  The kernel writes 32 B per sample and reads 32 B per
time sample per group of detectors; the record gives its written GB/s beside the 6.29 TB/s copy ceiling of the part
(profiles/r01_copy_ceiling.txt).  Before timing, the two variants are compared once (largest great-circle separation and response
difference), so the record says the torch form computes the same thing.  Prints one JSON line.  Not a test and not the
benchmark: no threshold."""
import argparse
import faulthandler
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import pixell_jl_amd as pj  # noqa: E402

COPY_CEILING_TBS = 6.29


def expand_torch(q_bore, q_det, gamma):
    """The definition of pxl_pointing_expand_f64 in torch elementwise operations: (D, T) broadcasts, then (D * T, 2) outputs."""
    q = pj.quat_mul(q_bore[None, :, :], q_det[:, None, :])
    bad = ~(torch.isfinite(q_bore).all(-1)[None, :] & torch.isfinite(q_det).all(-1)[:, None] & torch.isfinite(gamma)[:, None])
    bad |= (q_bore == 0).all(-1)[None, :] | (q_det == 0).all(-1)[:, None]
    w, x, y, z = q.unbind(-1)
    nx, ny, nz = 2 * (x * z + w * y), 2 * (y * z - w * x), w * w - x * x - y * y + z * z
    ex, ey, ez = w * w + x * x - y * y - z * z, 2 * (x * y + w * z), 2 * (x * z - w * y)
    h = torch.sqrt(nx * nx + ny * ny)
    pole = h == 0
    ra = torch.where(pole, torch.zeros_like(h), torch.atan2(ny + 0.0, nx))
    dec = torch.atan2(nz, h)
    nn = torch.sqrt(h * h + nz * nz)
    hs = torch.where(pole, torch.ones_like(h), h)
    east_x, east_y = torch.where(pole, torch.zeros_like(h), -ny / hs), torch.where(pole, torch.ones_like(h), nx / hs)
    # north = n^ x east, east_z = 0
    north_x, north_y, north_z = -(nz / nn) * east_y, (nz / nn) * east_x, (nx / nn) * east_y - (ny / nn) * east_x
    c, s = ex * north_x + ey * north_y + ez * north_z, ex * east_x + ey * east_y
    d = c * c + s * s
    g = gamma[:, None]
    nan = torch.full_like(h, float("nan"))
    sky = torch.stack((torch.where(bad, nan, ra), torch.where(bad, nan, dec)), dim=-1).reshape(-1, 2)
    resp = torch.stack((torch.where(bad, nan, g * (c * c - s * s) / d), torch.where(bad, nan, g * (2 * c * s) / d)), dim=-1).reshape(-1, 2)
    return sky, resp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=10 ** 5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--burst", type=int, default=3, help="timed calls per variant and round, behind one untimed call")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds one burst may take before the process is ended")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    assert args.burst >= 3 and args.rounds >= 1
    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda:0")
    nd, nt = args.dets, args.samples
    n = nd * nt
    gen = torch.Generator(device="cpu").manual_seed(416)
    q_bore = torch.randn((nt, 4), dtype=torch.float64, generator=gen)
    q_det = torch.randn((nd, 4), dtype=torch.float64, generator=gen)
    q_bore, q_det = (q_bore / q_bore.norm(dim=1, keepdim=True)).to(dev), (q_det / q_det.norm(dim=1, keepdim=True)).to(dev)
    gamma = torch.rand((nd,), dtype=torch.float64, generator=gen).to(dev)
    sky = torch.empty((n, 2), dtype=torch.float64, device=dev)
    resp = torch.empty((n, 2), dtype=torch.float64, device=dev)

    faulthandler.dump_traceback_later(args.step_limit, exit=True)
    pj.expand_pointing(q_bore, q_det, gamma, out_sky=sky, out_resp=resp)
    tsky, tresp = expand_torch(q_bore, q_det, gamma)
    chord = torch.sqrt((torch.cos(sky[:, 1]) * torch.cos(sky[:, 0]) - torch.cos(tsky[:, 1]) * torch.cos(tsky[:, 0])) ** 2
                       + (torch.cos(sky[:, 1]) * torch.sin(sky[:, 0]) - torch.cos(tsky[:, 1]) * torch.sin(tsky[:, 0])) ** 2
                       + (torch.sin(sky[:, 1]) - torch.sin(tsky[:, 1])) ** 2)
    agree = {"max_separation_rad": float(chord.max()), "max_response_difference_times_h": float(((resp - tresp).abs().amax(dim=1) * torch.cos(tsky[:, 1])).max())}
    del tsky, tresp, chord
    torch.cuda.synchronize()
    faulthandler.cancel_dump_traceback_later()

    variants = {"expand_pointing": lambda: pj.expand_pointing(q_bore, q_det, gamma, out_sky=sky, out_resp=resp),
                "torch_elementwise": lambda: expand_torch(q_bore, q_det, gamma)}
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
            print("%s: %s ms" % (name, ", ".join("%.3f" % t for t in times[name][-args.burst:])), file=sys.stderr, flush=True)
    rec = {"dets": nd, "samples": nt, "points": n, "rounds": args.rounds, "burst": args.burst, "device": torch.cuda.get_device_name(dev),
           "agreement": agree, "copy_ceiling_tbs": COPY_CEILING_TBS}
    for name, t in times.items():
        t = sorted(t)
        rec[name] = {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}
    ms = rec["expand_pointing"]["median_ms"]
    rec["written_gbs"] = round(32.0 * n / (ms * 1e-3) / 1e9, 1)
    rec["written_over_copy_ceiling"] = round(rec["written_gbs"] / (COPY_CEILING_TBS * 1e3), 3)
    rec["torch_over_kernel"] = round(rec["torch_elementwise"]["median_ms"] / ms, 1)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
