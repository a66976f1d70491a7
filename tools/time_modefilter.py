#!/usr/bin/env python3
"""Time the detector-mode filter pj.modefilter_tod against the torch composition it replaces, on the same build:
--dets x --samples samples (1000 x 10^5) in one group and in ten equal groups, K = 1 and 3 modes, random weights with one sample
in ten cut.

The composition is batched normal equations over the T time samples of each group, with F the group's (D_g, K) couplings and the
timestream viewed as (n_grp, D_g, T):

    G = w^T @ (F (x) F)   (one batched matmul to (n_grp, T, K, K)),   b = (w * d)^T @ F,   c = torch.linalg.solve(G, b),
    out = d - F @ c^T

-- it materialises (T, K, K) systems, cannot cut a NaN sample (0 * NaN), has no truncation rule, and its G is not the library's
bit for bit.  What is timed:

    fused        modefilter_tod(tod, modes, w, grp_start, out=out)               (grp_start's upload included)
    fused_place  the same in place (out = tod): no second buffer
    compose      the four torch steps above

Beside each time the record gives the bytes the call must move -- d and wfit read, out written: 24 B per sample; whether the second
read of d comes from on chip is not known (a group tile is D_g x C x 8 B) -- and the time those bytes take at the 6.29 TB/s copy
ceiling of DESIGN.md 6.

    python tools/time_modefilter.py [--dets 1000] [--samples 100000] [--groups 1 10] [--modes 1 3] [--burst 5] [--step-limit 120]
                                    [--out profiles/modefilter_times.json]

EVERY GPU STEP RUNS UNDER ITS OWN TIME LIMIT: the parent process never opens the GPU; each (groups, K) configuration is one fresh
child process (this file with --child) under `timeout -k 10 <step-limit>`, which times its variants in bursts of one untimed
call plus `burst` calls between hipEvents and prints one JSON line.  The first child that fails, is killed or times out ends the
run: nothing more is started on the GPU and nothing is retried.  Prints one JSON line.  Not a test and not the benchmark."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_TBS = 6.29


def child(args):
    import torch

    import pixell_jl_amd as pj

    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda:0")
    nd, nt, ng, K = args.dets, args.samples, args.child[0], args.child[1]
    assert nd % ng == 0
    dg = nd // ng
    f64 = dict(dtype=torch.float64, device=dev)
    tod = torch.empty((nd, nt), **f64)
    pj.fill_random_(tod.view(-1), 51)
    w = torch.empty((nd, nt), **f64)
    pj.fill_random_(w.view(-1), 52, kind="uniform")
    w = (w * (w > 0.1)).contiguous()                                    # one sample in ten cut
    modes = torch.empty((nd, K), **f64)
    pj.fill_random_(modes.view(-1), 53)
    modes[:, 0] = 1.0
    out = torch.empty_like(tod)
    work = tod.clone()
    grp = list(range(0, nd + 1, dg))
    Fg = modes.view(ng, dg, K)
    FF = (Fg[:, :, :, None] * Fg[:, :, None, :]).reshape(ng, dg, K * K).contiguous()
    torch.cuda.synchronize()

    def compose():
        wv, dv = w.view(ng, dg, nt), tod.view(ng, dg, nt)
        G = (wv.transpose(1, 2) @ FF).view(ng, nt, K, K)
        b = (wv * dv).transpose(1, 2) @ Fg
        c = torch.linalg.solve(G, b)
        return (dv - Fg @ c.transpose(1, 2)).view(nd, nt)

    variants = {"fused": lambda: pj.modefilter_tod(tod, modes, w=w, grp_start=grp, out=out),
                "fused_place": lambda: pj.modefilter_tod(work, modes, w=w, grp_start=grp, out=work),
                "compose": compose}
    check = float((pj.modefilter_tod(tod, modes, w=w, grp_start=grp) - compose()).abs().max())
    torch.cuda.synchronize()
    nbytes = 24 * nd * nt
    rec = {"groups": ng, "modes": K, "max_abs_fused_minus_compose": check}
    for name, run in variants.items():
        run()                                                # untimed: the burst's timed calls follow a call of their own kind
        times = []
        for _b in range(args.burst):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        print("groups %d K %d %s: %s ms" % (ng, K, name, ", ".join("%.3f" % t for t in times)), file=sys.stderr, flush=True)
        t = sorted(times)
        rec[name] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                     "TBs_of_bytes_moved": round(nbytes / (t[len(t) // 2] * 1e-3) / 1e12, 3)}
    rec["compose_over_fused"] = round(rec["compose"]["median_ms"] / rec["fused"]["median_ms"], 3)
    rec["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=10 ** 5, help="time samples per detector")
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--modes", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--burst", type=int, default=5, help="timed calls per variant, behind one untimed call")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds one configuration's child process may take")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--child", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.burst >= 3
    if args.child:
        return child(args)
    nbytes = 24 * args.dets * args.samples
    rec = {"dets": args.dets, "samples": args.samples, "burst": args.burst, "rounds": 1, "bytes_moved": nbytes,
           "copy_ceiling_TBs": COPY_CEILING_TBS, "ms_at_copy_ceiling": round(nbytes / (COPY_CEILING_TBS * 1e12) * 1e3, 4), "runs": []}
    for ng in args.groups:
        for K in args.modes:
            cmd = ["timeout", "-k", "10", str(args.step_limit), sys.executable, os.path.abspath(__file__), "--dets", str(args.dets), "--samples",
                   str(args.samples), "--burst", str(args.burst), "--child", str(ng), str(K)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                sys.exit("groups %d K %d ended with status %d: nothing more is started" % (ng, K, r.returncode))
            one = json.loads(r.stdout.strip().splitlines()[-1])
            rec["device"] = one.pop("device")
            rec["runs"].append(one)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
