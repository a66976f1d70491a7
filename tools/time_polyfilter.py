#!/usr/bin/env python3
"""Time the per-scan polynomial filter pj.polyfilter_tod against the torch composition it replaces, on the same
build and in one process: --dets x --samples samples (1000 x 10^5) in segments of --seg-len (2000) samples, orders 1 and 5,
random weights with one sample in ten cut.

The composition is batched normal equations on EQUAL-length segments, the only case torch does without padding: with F the
(L, p) Legendre basis and the timestream viewed as (D, S, L),

    G = w @ (F (x) F)   (one matmul to (D, S, p, p)),   b = (w * d) @ F,   c = torch.linalg.solve(G, b),   out = d - c @ F^T

-- it cannot cut a NaN sample (0 * NaN), and its G is not the library's bit for bit.  What is timed:

    fused        polyfilter_tod(tod, seg_start, order, w, out=out)               (seg_start's upload included)
    fused_place  the same in place (out = tod): no second buffer
    compose      the four torch steps above

Beside each time the record gives the bytes the call must move -- d and wfit read, out written: 24 B per sample; the second
read of d should come from L2 -- and the time those bytes take at the 6.29 TB/s copy ceiling of DESIGN.md 6.

    python tools/time_polyfilter.py [--dets 1000] [--samples 100000] [--seg-len 2000] [--orders 1 5] [--rounds 1] [--burst 5]
                                    [--step-limit 120] [--out profiles/polyfilter_times.json]

Each variant is timed in bursts of one untimed call plus `burst` calls between hipEvents (as tools/time_destripe.py does), the
variants interleaved over `rounds`; a watchdog ends the process, with a traceback, if one burst takes longer than --step-limit
seconds; nothing is retried.  Prints one JSON line.  Not a test and not the benchmark: no threshold."""
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


def legendre_basis(L, order, dev):
    """(L, order + 1): the library's x_j = ((2j + 1) - L) / L and recurrence."""
    j = torch.arange(L, dtype=torch.float64, device=dev)
    x = ((2 * j + 1) - L) / L
    P = [torch.ones_like(x), x]
    for n in range(1, order):
        P.append(((2 * n + 1) * x * P[n] - n * P[n - 1]) / (n + 1))
    return torch.stack(P[:order + 1], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=10 ** 5, help="time samples per detector")
    ap.add_argument("--seg-len", type=int, default=2000)
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--burst", type=int, default=5, help="timed calls per variant and round, behind one untimed call")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds one burst may take before the process is ended")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    assert args.burst >= 3 and args.rounds >= 1 and args.samples % args.seg_len == 0
    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda:0")
    nd, nt, L = args.dets, args.samples, args.seg_len
    ns = nt // L
    f64 = dict(dtype=torch.float64, device=dev)
    tod = torch.empty((nd, nt), **f64)
    pj.fill_random_(tod.view(-1), 51)
    w = torch.empty((nd, nt), **f64)
    pj.fill_random_(w.view(-1), 52, kind="uniform")
    w = (w * (w > 0.1)).contiguous()                                    # one sample in ten cut
    out = torch.empty_like(tod)
    work = tod.clone()
    seg = list(range(0, nt + 1, L))
    torch.cuda.synchronize()

    variants, check = {}, {}
    for order in args.orders:
        F = legendre_basis(L, order, dev)
        FF = (F[:, :, None] * F[:, None, :]).reshape(L, -1).contiguous()
        p = order + 1

        def compose(F=F, FF=FF, p=p):
            wv, dv = w.view(nd, ns, L), tod.view(nd, ns, L)
            G = (wv @ FF).view(nd, ns, p, p)
            b = (wv * dv) @ F
            c = torch.linalg.solve(G, b)
            return (dv - c @ F.T).view(nd, nt)

        variants["fused_order%d" % order] = lambda order=order: pj.polyfilter_tod(tod, seg, order, w=w, out=out)
        variants["fused_place_order%d" % order] = lambda order=order: pj.polyfilter_tod(work, seg, order, w=w, out=work)
        variants["compose_order%d" % order] = compose
        check[order] = float((pj.polyfilter_tod(tod, seg, order, w=w) - compose()).abs().max())
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
            print("%s: %s ms" % (name, ", ".join("%.3f" % t for t in times[name][-args.burst:])), file=sys.stderr, flush=True)
    nbytes = 24 * nd * nt
    rec = {"dets": nd, "samples": nt, "seg_len": L, "rounds": args.rounds, "burst": args.burst, "device": torch.cuda.get_device_name(dev),
           "bytes_moved": nbytes, "copy_ceiling_TBs": COPY_CEILING_TBS, "ms_at_copy_ceiling": round(nbytes / (COPY_CEILING_TBS * 1e12) * 1e3, 4)}
    for name, t in times.items():
        t = sorted(t)
        rec[name] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                     "TBs_of_bytes_moved": round(nbytes / (t[len(t) // 2] * 1e-3) / 1e12, 3)}
    for order in args.orders:
        rec["compose_over_fused_order%d" % order] = round(rec["compose_order%d" % order]["median_ms"] / rec["fused_order%d" % order]["median_ms"], 3)
        rec["max_abs_fused_minus_compose_order%d" % order] = check[order]
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
