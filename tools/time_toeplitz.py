#!/usr/bin/env python3
"""Time pj.toeplitz_tod against the torch FFT form of the same operator, on the same build: --dets x --samples
samples (1000 x 10^5) in scans of --seg-len (2000), one sample in ten cut, at every --lams (0 16 128 1024 4096).  It stands beside
tools/time_tod_filters.py, whose variants (in place, fit outputs) this operator does not have.

What is timed, per lambda:

    fused    pj.toeplitz_tod(tod, kernel, seg_start, w=g, out=out)                    (the offsets' upload included)
    fft      per scan, g * irfft(rfft(g * x, n) * rfft(kernel_n), n)[:L], n the power of two >= L + lambda: the linear convolution
             of the zero-padded scan with the symmetric kernel laid out circularly; rfft(kernel_n) is made once, outside the timed
             calls, as a map-maker would make it.  It is not bit-reproducible against the definition and multiplies a NaN under a
             cut by zero, which is a NaN.

Beside each time: the bytes the call must move (x and wlive read, out written: 24 B per sample) as a share of the 6.29 TB/s copy
ceiling of DESIGN.md 6; and the Float64 operations of the definition, 3 lambda + 1 per sample (an add, a multiply and an add per
tap, none fused), per second and as a share of the 78.6 TFLOP/s vector peak of AMD's specification -- which counts a fused
multiply-add as two, so code that may not fuse can reach half of it.

    python tools/time_toeplitz.py [--dets 1000] [--samples 100000] [--seg-len 2000] [--lams 0 16 128 1024 4096]
                                  [--rounds 1] [--burst 5] [--step-limit 120] [--out profiles/toeplitz_times.json]

EVERY GPU STEP RUNS UNDER ITS OWN TIME LIMIT: the parent process never opens the GPU; each lambda is one fresh child process (this
file with --child) under `timeout -k 10 <step-limit>`, which times its variants in bursts of one untimed call plus `burst` calls
between hipEvents, the variants interleaved over `rounds`, and prints one JSON line.  The first child that fails, is killed or
times out ends the run: nothing more is started on the GPU and nothing is retried.  Prints one JSON line, the record
profiles/toeplitz_times.json holds.  Not a test and not the benchmark: no threshold."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING_TBS = 6.29
FP64_VECTOR_PEAK_TFLOPS = 78.6


def child(args):
    """One lambda: {"device", "lam", variant: {median_ms, min_ms, max_ms}, "fft_over_fused", "max_abs_fused_minus_fft"}."""
    import numpy as np
    import torch

    import pixell_jl_amd as pj

    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda:0")
    nd, nt, L, lam = args.dets, args.samples, args.seg_len, args.child
    ns = nt // L
    tod = torch.empty((nd, nt), dtype=torch.float64, device=dev)
    pj.fill_random_(tod.view(-1), 51)
    g = torch.empty((nd, nt), dtype=torch.float64, device=dev)
    pj.fill_random_(g.view(-1), 52, kind="uniform")
    g = (g > 0.1).to(torch.float64).contiguous()                        # one sample in ten cut
    f = np.fft.rfftfreq(8192)
    f[0] = f[1]
    kern = pj.noise_kernel_from_psd(1.0 + (0.01 / f) ** 2, lam).to(dev)  # (lam + 1,): the same kernel for every detector
    seg = list(range(0, nt + 1, L))
    out = torch.empty_like(tod)
    n = 1
    while n < L + lam:
        n *= 2
    kn = torch.zeros((n,), dtype=torch.float64, device=dev)
    kn[:lam + 1] = kern
    if lam:
        kn[n - lam:] = kern[1:].flip(0)
    K = torch.fft.rfft(kn)

    def fft():
        gv = g.view(nd, ns, L)
        return (gv * torch.fft.irfft(torch.fft.rfft(gv * tod.view(nd, ns, L), n=n) * K, n=n)[..., :L]).view(nd, nt)

    variants = {"fused": lambda: pj.toeplitz_tod(tod, kern, seg, w=g, out=out), "fft": fft}
    torch.cuda.synchronize()
    rec = {"lam": lam, "fft_length": n, "max_abs_fused_minus_fft": float((variants["fused"]() - fft()).abs().max())}
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
            print("toeplitz lambda %d %s: %s ms" % (lam, name, ", ".join("%.3f" % t for t in times[name][-args.burst:])), file=sys.stderr, flush=True)
    for name, t in times.items():
        t = sorted(t)
        rec[name] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4)}
    ms = rec["fused"]["median_ms"]
    flops = (3 * lam + 1) * nd * nt
    rec["fused"].update({"share_of_copy_ceiling": round(24 * nd * nt / (ms * 1e-3) / (COPY_CEILING_TBS * 1e12), 4),
                         "taps_per_s": round((lam + 1) * nd * nt / (ms * 1e-3), 1), "fp64_flops_per_s": round(flops / (ms * 1e-3), 1),
                         "share_of_fp64_vector_peak": round(flops / (ms * 1e-3) / (FP64_VECTOR_PEAK_TFLOPS * 1e12), 4)})
    rec["fft_over_fused"] = round(rec["fft"]["median_ms"] / ms, 3)
    rec["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=10 ** 5, help="time samples per detector")
    ap.add_argument("--seg-len", type=int, default=2000, help="samples per scan")
    ap.add_argument("--lams", type=int, nargs="+", default=[0, 16, 128, 1024, 4096])
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--burst", type=int, default=5, help="timed calls per variant and round, behind one untimed call")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds one lambda's child process may take")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.burst >= 3 and args.rounds >= 1 and args.samples % args.seg_len == 0
    if args.child is not None:
        return child(args)
    nbytes = 24 * args.dets * args.samples
    rec = {"dets": args.dets, "samples": args.samples, "seg_len": args.seg_len, "rounds": args.rounds, "burst": args.burst, "bytes_moved": nbytes,
           "copy_ceiling_TBs": COPY_CEILING_TBS, "ms_at_copy_ceiling": round(nbytes / (COPY_CEILING_TBS * 1e12) * 1e3, 4),
           "fp64_vector_peak_TFLOPs": FP64_VECTOR_PEAK_TFLOPS, "runs": []}
    for lam in args.lams:
        cmd = ["timeout", "-k", "10", str(args.step_limit), sys.executable, os.path.abspath(__file__), "--dets", str(args.dets), "--samples",
               str(args.samples), "--seg-len", str(args.seg_len), "--rounds", str(args.rounds), "--burst", str(args.burst), "--child", str(lam)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit("lambda %d ended with status %d: nothing more is started" % (lam, r.returncode))
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
