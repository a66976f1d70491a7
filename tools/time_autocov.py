#!/usr/bin/env python3
"""Time pj.autocov_tod against its three yardsticks on the same build and the same data: --dets x --samples samples
(1000 x 10^5) in scans of --seg-len (2000), one sample in ten cut, at every --lams (0 16 128 1024 4096).  tools/time_toeplitz.py's
protocol.

What is timed, per lambda:

    autocov   pj.autocov_tod(tod, lam, seg_start, w=g)                  sums and pairs (the offsets' upload and the outputs' allocation included)
    sums      pj.autocov_tod(tod, lam, seg_start, w=g, return_pairs=False)
    toeplitz  pj.toeplitz_tod(tod, kernel, seg_start, w=g, out=out)     the same products with one more add each, plus 8 B per sample written
    fft       per scan irfft(|rfft(g * x, n)|^2, n)[:lam + 1], n the power of two >= L + lam, summed over the scans: the zero-filled
              autocorrelation.  Not bit-reproducible, and it multiplies a NaN under a cut by zero, which is a NaN.  (pairs would be a
              second transform of g; it is not timed.)

Beside autocov's time: the 16 B per sample it must read (x and wlive) as a share of the 6.29 TB/s copy ceiling of DESIGN.md 6; and the
Float64 operations of the definition, a multiply and an add per pair -- counted for every (sample, lag) inside a scan's length, 2 (lam +
1) per sample less the pairs past the scans' ends -- per second and as a share of the 78.6 TFLOP/s vector peak, which counts a fused
multiply-add as two, so code that may not fuse can reach half of it.

    python tools/time_autocov.py [--dets 1000] [--samples 100000] [--seg-len 2000] [--lams 0 16 128 1024 4096]
                                 [--rounds 1] [--burst 5] [--step-limit 120] [--out profiles/autocov_times.json]

EVERY GPU STEP RUNS UNDER ITS OWN TIME LIMIT: the parent process never opens the GPU; each lambda is one fresh child process (this
file with --child) under `timeout -k 10 <step-limit>`, which times its variants in bursts of one untimed call plus `burst` calls
between hipEvents, the variants interleaved over `rounds`, and prints one JSON line.  The first child that fails, is killed or
times out ends the run: nothing more is started on the GPU and nothing is retried.  Prints one JSON line, the record
profiles/autocov_times.json holds.  Not a test and not the benchmark: no threshold."""
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
    """One lambda: {"device", "lam", variant: {median_ms, min_ms, max_ms}, ratios, "max_rel_autocov_minus_fft"}."""
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
    kern = pj.noise_kernel_from_psd(1.0 + (0.01 / f) ** 2, lam).to(dev)
    seg = list(range(0, nt + 1, L))
    out = torch.empty_like(tod)
    n = 1
    while n < L + lam:
        n *= 2

    def fft():
        z = torch.fft.rfft((g * tod).view(nd, ns, L), n=n)
        return torch.fft.irfft(z.real * z.real + z.imag * z.imag, n=n)[..., :lam + 1].sum(dim=1)

    variants = {"autocov": lambda: pj.autocov_tod(tod, lam, seg, w=g), "sums": lambda: pj.autocov_tod(tod, lam, seg, w=g, return_pairs=False),
                "toeplitz": lambda: pj.toeplitz_tod(tod, kern, seg, w=g, out=out), "fft": fft}
    torch.cuda.synchronize()
    sums, pairs = variants["autocov"]()
    reach = min(lam + 1, L)                                              # the lags a scan of L samples holds; the rest are +0.0
    rec = {"lam": lam, "fft_length": n,
           "max_rel_autocov_minus_fft": float(((sums - fft())[:, :reach].abs().max(dim=1).values / sums[:, 0]).max())}
    assert bool((pairs[:, reach:] == 0).all()) and bool((sums[:, reach:] == 0).all())
    del sums, pairs
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
            print("autocov lambda %d %s: %s ms" % (lam, name, ", ".join("%.3f" % t for t in times[name][-args.burst:])), file=sys.stderr, flush=True)
    for name, t in times.items():
        t = sorted(t)
        rec[name] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4), "timed_calls": len(t)}
    ms = rec["autocov"]["median_ms"]
    products = nd * ns * sum(L - k for k in range(reach))
    rec["autocov"].update({"share_of_copy_ceiling": round(16 * nd * nt / (ms * 1e-3) / (COPY_CEILING_TBS * 1e12), 4),
                           "products_per_s": round(products / (ms * 1e-3), 1), "fp64_flops_per_s": round(2 * products / (ms * 1e-3), 1),
                           "share_of_fp64_vector_peak": round(2 * products / (ms * 1e-3) / (FP64_VECTOR_PEAK_TFLOPS * 1e12), 4)})
    rec["toeplitz_over_autocov"] = round(rec["toeplitz"]["median_ms"] / ms, 3)
    rec["fft_over_autocov"] = round(rec["fft"]["median_ms"] / ms, 3)
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
    nbytes = 16 * args.dets * args.samples
    rec = {"dets": args.dets, "samples": args.samples, "seg_len": args.seg_len, "rounds": args.rounds, "burst": args.burst, "bytes_read": nbytes,
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
