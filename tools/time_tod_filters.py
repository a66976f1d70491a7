#!/usr/bin/env python3
"""Time a timestream filter against the torch composition it replaces, on the same build: --dets x --samples samples (1000 x 10^5),
random weights with one sample in ten cut.

--filter poly: pj.polyfilter_tod, segments of --seg-len (2000) samples, orders --orders (1 and 5).  The composition
is batched normal equations on EQUAL-length segments, the only case torch does without padding: with F the (L, p) Legendre basis and
the timestream viewed as (D, S, L),

    G = w @ (F (x) F)   (one matmul to (D, S, p, p)),   b = (w * d) @ F,   c = torch.linalg.solve(G, b),   out = d - c @ F^T

--filter mode: pj.modefilter_tod, in --groups (one and ten) equal groups, K = --modes (1 and 3).  The composition is
batched normal equations over the T time samples of each group, with F the group's (D_g, K) couplings and the timestream viewed as
(n_grp, D_g, T):

    G = w^T @ (F (x) F)   (one batched matmul to (n_grp, T, K, K)),   b = (w * d)^T @ F,   c = torch.linalg.solve(G, b),
    out = d - F @ c^T

-- which materialises (T, K, K) systems and has no truncation rule.

--filter bin: pj.binfilter_tod on the plan of a triangle-wave scan of --seg-len samples per sweep (1000, 2000 and
8000) binned by position into --bins (200) bins: a sweep stays seg-len / bins samples in a bin (5, 10 and 40).  The composition is

    s = zeros(D, n_bin).index_add_(1, index, w * d),   n = zeros(D, n_bin).index_add_(1, index, w),   c = s / n,
    out = d - c.index_select(1, index)

-- two passes of atomics whose sums are not bit-reproducible.  Beside the three variants below, fused_contig: the library call with a
plan whose bins are contiguous in time (an identity order, T / bins samples per bin), the gather-free best case with the traffic of
pj.polyfilter_tod at order 0.  The plan is made once, outside the timed calls, as a map-maker makes it.

No composition can cut a NaN sample (0 * NaN), and none has the library's sums bit for bit.  What is timed:

    fused        the library call with out=out                                   (the offsets' upload included)
    fused_place  the same in place (out = tod): no second buffer
    compose      the torch steps above

Beside each time the record gives the bytes the call must move -- d and wfit read, out written: 24 B per sample; whether the second
read of d comes from on chip depends on the item (a segment should; a group tile is D_g x C x 8 B) -- and the time those bytes take at
the 6.29 TB/s copy ceiling of DESIGN.md 6.

    python tools/time_tod_filters.py --filter poly [--dets 1000] [--samples 100000] [--seg-len 2000] [--orders 1 5]
    python tools/time_tod_filters.py --filter mode [--dets 1000] [--samples 100000] [--groups 1 10] [--modes 1 3]
    python tools/time_tod_filters.py --filter bin [--dets 1000] [--samples 100000] [--seg-len 1000 2000 8000] [--bins 200]
                                     [--rounds 1] [--burst 5] [--step-limit 120] [--out profiles/<poly|mode|bin>filter_times.json]

EVERY GPU STEP RUNS UNDER ITS OWN TIME LIMIT: the parent process never opens the GPU; each configuration (an order; a (groups, K)
pair; a sweep length) is one fresh child process (this file with --child) under `timeout -k 10 <step-limit>`, which times its variants in bursts
of one untimed call plus `burst` calls between hipEvents, the variants interleaved over `rounds`, and prints one JSON line.  The
first child that fails, is killed or times out ends the run: nothing more is started on the GPU and nothing is retried.  Prints
one JSON line, with the keys profiles/polyfilter_times.json, profiles/modefilter_times.json and profiles/binfilter_times.json have.  Not a test and not the
benchmark: no threshold."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_TBS = 6.29


def legendre_basis(torch, L, order, dev):
    """(L, order + 1): the library's x_j = ((2j + 1) - L) / L and recurrence."""
    j = torch.arange(L, dtype=torch.float64, device=dev)
    x = ((2 * j + 1) - L) / L
    P = [torch.ones_like(x), x]
    for n in range(1, order):
        P.append(((2 * n + 1) * x * P[n] - n * P[n - 1]) / (n + 1))
    return torch.stack(P[:order + 1], dim=1)


def poly_variants(torch, pj, args, order, tod, w, out, work):
    nd, nt, L = args.dets, args.samples, args.seg_len
    ns = nt // L
    seg = list(range(0, nt + 1, L))
    F = legendre_basis(torch, L, order, tod.device)
    FF = (F[:, :, None] * F[:, None, :]).reshape(L, -1).contiguous()
    p = order + 1

    def compose():
        wv, dv = w.view(nd, ns, L), tod.view(nd, ns, L)
        G = (wv @ FF).view(nd, ns, p, p)
        b = (wv * dv) @ F
        c = torch.linalg.solve(G, b)
        return (dv - c @ F.T).view(nd, nt)

    return {"fused": lambda: pj.polyfilter_tod(tod, seg, order, w=w, out=out),
            "fused_place": lambda: pj.polyfilter_tod(work, seg, order, w=w, out=work),
            "compose": compose}, lambda: pj.polyfilter_tod(tod, seg, order, w=w)


def mode_variants(torch, pj, args, ng, K, tod, w, out, work):
    nd, nt = args.dets, args.samples
    assert nd % ng == 0
    dg = nd // ng
    modes = torch.empty((nd, K), dtype=torch.float64, device=tod.device)
    pj.fill_random_(modes.view(-1), 53)
    modes[:, 0] = 1.0
    grp = list(range(0, nd + 1, dg))
    Fg = modes.view(ng, dg, K)
    FF = (Fg[:, :, :, None] * Fg[:, :, None, :]).reshape(ng, dg, K * K).contiguous()

    def compose():
        wv, dv = w.view(ng, dg, nt), tod.view(ng, dg, nt)
        G = (wv.transpose(1, 2) @ FF).view(ng, nt, K, K)
        b = (wv * dv).transpose(1, 2) @ Fg
        c = torch.linalg.solve(G, b)
        return (dv - Fg @ c.transpose(1, 2)).view(nd, nt)

    return {"fused": lambda: pj.modefilter_tod(tod, modes, w=w, grp_start=grp, out=out),
            "fused_place": lambda: pj.modefilter_tod(work, modes, w=w, grp_start=grp, out=work),
            "compose": compose}, lambda: pj.modefilter_tod(tod, modes, w=w, grp_start=grp)


def bin_variants(torch, pj, args, L, tod, w, out, work):
    nd, nt, nb = args.dets, args.samples, args.bins
    t = torch.arange(nt, device=tod.device)
    ph = t % (2 * L)
    pos = torch.where(ph < L, ph, 2 * L - 1 - ph)                        # the triangle wave: 0 .. L - 1 and back
    index = (pos * nb) // L
    plan = pj.bin_plan(index, nb)
    contig = pj.bin_plan((t * nb) // nt, nb)                             # bins that are contiguous in time: an identity order

    def compose():
        s = torch.zeros((nd, nb), dtype=torch.float64, device=tod.device).index_add_(1, index, w * tod)
        n = torch.zeros((nd, nb), dtype=torch.float64, device=tod.device).index_add_(1, index, w)
        return tod - (s / n).index_select(1, index)

    return {"fused": lambda: pj.binfilter_tod(tod, plan, w=w, out=out),
            "fused_place": lambda: pj.binfilter_tod(work, plan, w=w, out=work),
            "compose": compose,
            "fused_contig": lambda: pj.binfilter_tod(tod, contig, w=w, out=out)}, lambda: pj.binfilter_tod(tod, plan, w=w)


def child(args):
    """One configuration: {"device", variant: {median_ms, min_ms, max_ms, TBs_of_bytes_moved}, "compose_over_fused",
    "max_abs_fused_minus_compose"}."""
    import torch

    import pixell_jl_amd as pj

    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda:0")
    nd, nt = args.dets, args.samples
    tod = torch.empty((nd, nt), dtype=torch.float64, device=dev)
    pj.fill_random_(tod.view(-1), 51)
    w = torch.empty((nd, nt), dtype=torch.float64, device=dev)
    pj.fill_random_(w.view(-1), 52, kind="uniform")
    w = (w * (w > 0.1)).contiguous()                                    # one sample in ten cut
    out = torch.empty_like(tod)
    work = tod.clone()
    make = {"poly": poly_variants, "mode": mode_variants, "bin": bin_variants}[args.filter]
    variants, fused = make(torch, pj, args, *args.child, tod, w, out, work)
    torch.cuda.synchronize()
    rec = {"max_abs_fused_minus_compose": float((fused() - variants["compose"]()).abs().max())}
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, run in variants.items():
            run()                                            # untimed: the burst's timed calls follow a call of their own kind
            for _b in range(args.burst):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
            print("%s %s %s: %s ms" % (args.filter, args.child, name, ", ".join("%.3f" % t for t in times[name][-args.burst:])), file=sys.stderr,
                  flush=True)
    nbytes = 24 * nd * nt
    for name, t in times.items():
        t = sorted(t)
        rec[name] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4),
                     "TBs_of_bytes_moved": round(nbytes / (t[len(t) // 2] * 1e-3) / 1e12, 3)}
    rec["compose_over_fused"] = round(rec["compose"]["median_ms"] / rec["fused"]["median_ms"], 3)
    rec["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filter", choices=["poly", "mode", "bin"], required=True)
    ap.add_argument("--dets", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=10 ** 5, help="time samples per detector")
    ap.add_argument("--seg-len", type=int, nargs="+", default=None, help="poly: samples per segment (2000); bin: samples per sweep, one run each (1000 2000 8000)")
    ap.add_argument("--bins", type=int, default=200, help="bin")
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 5], help="poly")
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 10], help="mode")
    ap.add_argument("--modes", type=int, nargs="+", default=[1, 3], help="mode")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--burst", type=int, default=5, help="timed calls per variant and round, behind one untimed call")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds one configuration's child process may take")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--child", type=int, nargs="+", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.burst >= 3 and args.rounds >= 1
    poly = args.filter == "poly"
    if args.filter == "bin":
        sweeps = args.seg_len or [1000, 2000, 8000]
    else:
        assert args.seg_len is None or len(args.seg_len) == 1
        sweeps, args.seg_len = None, (args.seg_len or [2000])[0]
    assert not poly or args.samples % args.seg_len == 0
    if args.child:
        return child(args)
    nbytes = 24 * args.dets * args.samples
    rec = {"dets": args.dets, "samples": args.samples}
    if poly:
        rec["seg_len"] = args.seg_len
    if sweeps:
        rec["bins"] = args.bins
    rec.update({"rounds": args.rounds, "burst": args.burst, "bytes_moved": nbytes, "copy_ceiling_TBs": COPY_CEILING_TBS,
                "ms_at_copy_ceiling": round(nbytes / (COPY_CEILING_TBS * 1e12) * 1e3, 4)})
    if not poly:
        rec["runs"] = []
    configs = [(o,) for o in args.orders] if poly else [(L,) for L in sweeps] if sweeps else [(ng, K) for ng in args.groups for K in args.modes]
    for cfg in configs:
        cmd = ["timeout", "-k", "10", str(args.step_limit), sys.executable, os.path.abspath(__file__), "--filter", args.filter, "--dets", str(args.dets),
               "--samples", str(args.samples), "--seg-len", str(cfg[0] if sweeps else args.seg_len), "--bins", str(args.bins), "--rounds", str(args.rounds), "--burst", str(args.burst), "--child"]
        r = subprocess.run(cmd + [str(c) for c in cfg], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit("%s %s ended with status %d: nothing more is started" % (args.filter, cfg, r.returncode))
        one = json.loads(r.stdout.strip().splitlines()[-1])
        rec["device"] = one.pop("device")
        if poly:                                             # polyfilter_times.json's flat keys: every name ends in its order
            rec.update({"%s_order%d" % (name, cfg[0]): val for name, val in one.items()})
        elif sweeps:
            rec["runs"].append(dict(seg_len=cfg[0], samples_per_bin_and_sweep=cfg[0] / args.bins, **one))
        else:
            rec["runs"].append(dict(groups=cfg[0], modes=cfg[1], **one))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
