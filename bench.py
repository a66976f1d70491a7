#!/usr/bin/env python3
"""bench.py -- headline benchmark: Float64 CAR bilinear reprojection throughput (Mpix/s) and fraction of
the MI355X HBM roofline, at 1/2/4/8 GPUs of one node (strong scaling, dec-strip sharding, RCCL halo).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg4|cfg4x2|cfg3|cfg3s|cfg2|cfg5] [--full] [--dump-outputs DIR]

For N > 1 there is one rank per GPU.  Either launch them yourself,
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
or call `python bench.py --gpus N ...` from a bare shell: with no WORLD_SIZE in the environment the process starts
exactly that command as a child (before it has touched the GPU), relays the one JSON line and exits with its code.

A "step" is one pass of the hot path over the whole synthetic map (inputs resident in HBM): halo exchange
(N > 1) + coordinate-table build + reprojection of every component.  Rank 0 prints ONE JSON line.

Workloads (BASELINE.json configs; natural Clenshaw-Curtis shapes, ny = nx/2 + 1):
    cfg4 (default): (43200, 21601, 3) IQU -> same shape, half-pixel-shifted WCS; 16 B per output value.
                    This is the configuration north_star quotes the metric on ("full-sky 0.5-arcmin CAR
                    bilinear reprojection", ">= 6x strong scaling to 8 GPUs"); it fits one GPU (44.8 GB).
    cfg3: (21600, 10801) -> (43200, 21601) 2x refinement, 10 B per output pixel.
    cfg3s: (21600, 10801) -> same shape, half-pixel-shifted WCS (second workload), 16 B.
    cfg2: (4096, 2049) -> (8192, 4097) (Infinity-Cache resident; informational).
    cfg5: 1e9 scattered (ra, dec) points sampled from a (43200, 21601) map replicated per GPU.

Where the maps live (round 4): the headline's maps come from DecStripReprojector.alloc_maps() -- the library's default for a resident
source / destination pair (placement.place_pair_shifted): ONE allocation of exactly the pair's size whose destination lies across
a boundary between two of the HBM's memory classes; a scout allocation finds the boundaries with the library's store probe, a
ballast shifts the pair onto one, both go back to the driver before the call returns.  Nothing is kept beyond the two maps, and
nothing about this workload is timed.  (the 144-GiB-head-room placement is no longer the headline's; the plain
pair -- alloc_pair, --arena -- is a lottery between processes: 0.70-0.79 of 8 TB/s, profiles/r04_headline_policy.txt.)
--arena = alloc_pair (plain), --api-default = source torch.empty + destination pj.empty_map, --placed = pj.place_pair (144 GiB of
head-room: the best placement, rounds 1-3's headline policy), --two-allocations = two torch.empty; a --full run reports three
policies for every reprojection config (configs.*.api_default / .class_aware_placement / .plain_first_placement).

A plain run sets up, warms up, times the K steps and prints the line (metric, value, unit, higher_is_better, dtype, ms_per_step,
the roofline fraction from the timed steps' HIP events, ...); nothing else.  --dump-outputs DIR also writes, after the timed
steps, a fixed seeded sample of what the last timed step computed as DIR/<name>.npy (float64), so that two builds can be
compared output for output: inputs are seeded, identical from run to run for the same arguments.

--full adds, after the headline and outside its timed region: the oracle check of the timed output (also --check alone),
the `sustained` loop, the CPU oracle's rate for the same workload (cpu_baseline), and for N = 1, workload cfg4, the live
traffic passes under rocprofv3, a "configs" block with the other BASELINE configs measured in the same process (cfg2, cfg3,
cfg3s, cfg5 at 1e9 points: ms per step, kernel average, roofline fraction, oracle check), an "evaluators" block (posmap,
pix2sky!, sky2pix! on the GPU) and the CPU oracle's rates for the functions the reference has (cpu_baseline.posmap / .pix2sky
/ .sky2pix); for N > 1, workload cfg4, configs.cfg5.  --no-configs, --no-traffic and --no-cpu-baseline trim a --full run.
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: required for RCCL P2P on this pool
# Thread placement of the cpu_baseline legs: NOT bound.  OMP_PROC_BIND would have to be set before libgomp loads (at `import
# torch`) and then pins this process's main thread to one CPU -- a mask that every child (the self-launched ranks, the rocprofv3
# passes) inherits.  The legs report the variables as they are (normally unset: threads float under the Linux scheduler).

import torch                      # noqa: E402
import torch.distributed as dist  # noqa: E402

import pixell_jl_amd as pj        # noqa: E402

HBM_PEAK_GBS = 8000.0             # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md


def baseline_metric():
    """BASELINE.json's metric string (the unit is its leading token, Mpix/s)."""
    try:
        with open(os.path.join(ROOT, "BASELINE.json")) as f:
            return json.load(f)["metric"]
    except Exception:
        return "Mpix/s CAR bilinear reproject (Float64) + % HBM roofline, 1/2/4/8 MI355X"


def workload_geometry(name):
    if name == "cfg4":
        shape_in, wcs_in = pj.fullsky_geometry(2 * math.pi / 43200, dims=(3,))
        shape_out = shape_in[:2]
        wcs_out = pj.CarClenshawCurtis(wcs_in.cdelt, (wcs_in.crpix[0] + 0.5, wcs_in.crpix[1] + 0.5), wcs_in.crval)
        desc = "cfg4: 43200x21601x3 IQU Float64 full-sky CAR -> same shape, half-pixel-shifted WCS (0.5 arcmin)"
    elif name == "cfg4x2":      # SURVEY 8(d) "secondary": the IQU map onto the 2x-refined grid (89.6 GB out)
        shape_in, wcs_in = pj.fullsky_geometry(2 * math.pi / 43200, dims=(3,))
        shape_out, wcs_out = pj.fullsky_geometry(2 * math.pi / 86400)
        desc = "cfg4x2: 43200x21601x3 IQU Float64 full-sky CAR -> 2x-refined 86400x43201x3 (0.25 arcmin)"
    elif name == "cfg3":
        shape_in, wcs_in = pj.fullsky_geometry(2 * math.pi / 21600)
        shape_out, wcs_out = pj.fullsky_geometry(2 * math.pi / 43200)
        desc = "cfg3: 21600x10801 I-only Float64 full-sky CAR -> 2x-refined 43200x21601"
    elif name == "cfg3s":       # SURVEY 8(d) config 3, second workload: same resolution, crval shifted by half a pixel in both axes
        shape_in, wcs_in = pj.fullsky_geometry(2 * math.pi / 21600)
        shape_out = shape_in[:2]
        wcs_out = pj.CarClenshawCurtis(wcs_in.cdelt, (wcs_in.crpix[0] + 0.5, wcs_in.crpix[1] + 0.5), wcs_in.crval)
        desc = "cfg3s: 21600x10801 I-only Float64 full-sky CAR -> same shape, half-pixel-shifted WCS (1 arcmin)"
    elif name == "cfg2":
        shape_in, wcs_in = pj.fullsky_geometry(2 * math.pi / 4096)
        shape_out, wcs_out = pj.fullsky_geometry(2 * math.pi / 8192)
        desc = "cfg2: 4096x2049 Float64 full-sky CAR -> 2x-refined 8192x4097 (cache resident)"
    elif name in ("down2", "down4", "up4"):     # other scale factors (diagnostics; not BASELINE configs)
        nin, nout = {"down2": (43200, 21600), "down4": (43200, 10800), "up4": (10800, 43200)}[name]
        shape_in, wcs_in = pj.fullsky_geometry(2 * math.pi / nin)
        shape_out, wcs_out = pj.fullsky_geometry(2 * math.pi / nout)
        desc = "%s: %dx%d -> %dx%d" % (name, shape_in[0], shape_in[1], shape_out[0], shape_out[1])
    else:
        raise ValueError(name)
    nc = shape_in[2] if len(shape_in) > 2 else 1
    return (shape_in[0], shape_in[1], nc), wcs_in, shape_out, wcs_out, desc


def fill_strip(sh, src, seed):
    """Deterministic N(0,1) map values keyed by (component, absolute pixel index): only the rows this rank
    OWNS are generated; halo rows must arrive through the exchange."""
    nx, ny, nc = sh.shape_in
    own_lo, own_hi = sh.own[sh.rank]
    sl = sh.own_slice()
    for c in range(nc):
        plane = src[c, sl, :]
        assert plane.is_contiguous()
        pj.fill_random_(plane, seed + c, offset=own_lo * nx, kind="normal")


def host_cpu_share():
    """What this process may really use of the host: hardware threads, physical cores, the affinity mask and the cgroup CPU quota
    (a GPU box hands a one-GPU job a share of a 128-thread host; 128 OpenMP threads inside a 16-CPU quota is how round 3 got a 7x
    'all-core' speed-up).  threads = min of the three, and that is what the all-core legs run with."""
    hw = os.cpu_count() or 1
    try:
        aff = len(os.sched_getaffinity(0))
    except Exception:
        aff = hw
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:                       # cgroup v2
            q, per = f.read().split()
        if q != "max":
            quota = float(q) / float(per)
    except Exception:
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:      # cgroup v1
                q = float(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = float(f.read())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    model, cores = None, set()
    try:
        phys = core = None
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name") and model is None:
                    model = line.split(":", 1)[1].strip()
                elif line.startswith("physical id"):
                    phys = line.split(":", 1)[1].strip()
                elif line.startswith("core id"):
                    core = line.split(":", 1)[1].strip()
                elif not line.strip():
                    if phys is not None and core is not None:
                        cores.add((phys, core))
                    phys = core = None
    except Exception:
        pass
    threads = max(1, min(hw, aff, int(math.ceil(quota)) if quota else hw))
    return {"threads": threads, "hardware_threads": hw, "physical_cores": len(cores) or None, "affinity_cpus": aff,
            "cgroup_cpu_quota": None if quota is None else round(quota, 2), "cpu_model": model,
            "OMP_PROC_BIND": os.environ.get("OMP_PROC_BIND"), "OMP_PLACES": os.environ.get("OMP_PLACES")}


def _cpu_median_rate(run, units, threads, runs=5):
    """median of >= 5 runs.  `run()` executes the oracle loop once into a caller-allocated output; the FIRST call
    is untimed -- it faults the output pages in (first touch by the threads that will write them: static OpenMP schedule, so every
    timed run finds its pages where its threads are) and warms the instruction cache.  Returns (units / s at the median, times)."""
    from oracle import oracle as O
    O.set_threads(threads)
    try:
        run()
        times = []
        for _ in range(runs):
            t0 = time.perf_counter()
            run()
            times.append(time.perf_counter() - t0)
    finally:
        O.set_threads(1)
    times.sort()
    return units / times[len(times) // 2], [round(t, 4) for t in times]


def cpu_baseline_reproject(shape_in, wcs_in, shape_out, wcs_out):
    """Time the CPU oracle (a C port of the reference arithmetic; the reference has no reprojection of its
    own and Julia is not installed) on a bounded strip of the same workload: one core (the reference's execution model) and
    every CPU this process may use, median of 5 runs each, output allocated and touched before the first timed run."""
    import numpy as np
    from oracle import oracle as O
    nx, ny, nc = shape_in
    nxo, nyo = shape_out
    mid = nyo // 2
    host = host_cpu_share()
    cores = max(1, min(O.max_threads(), host["threads"]))

    def leg(nrows, threads):
        lo = mid - nrows // 2
        s_lo, s_hi = O.reproject_src_rows(wcs_in, shape_in, wcs_out, shape_out, lo, nrows)
        src = np.random.default_rng(1234).random((nc, s_hi - s_lo, nx))
        out = np.empty((nc, nrows, nxo))
        rate, times = _cpu_median_rate(lambda: O.reproject(wcs_in, shape_in, src, wcs_out, shape_out, src_row0=s_lo, src_nrows=s_hi - s_lo,
                                                           dst_row0=lo, dst_nrows=nrows, out=out), nxo * nrows * nc, threads)
        return rate / 1e6, times

    # ~1 s per run: ~1.5e8 output values on one core (150 Mpix/s in round 3), scaled by a short calibration leg for all cores
    rows1 = min(max(8, int(1.5e8 / (nxo * nc))), nyo // 2)
    v1, t1 = leg(rows1, 1)
    vcal, _ = leg(rows1, cores) if cores > 1 else (v1, None)
    rowsN = max(rows1, min(int(1.0 * vcal * 1e6 / (nxo * nc)), nyo // 2, int(6e9 / (8 * nxo * nc))))
    vN, tN = leg(rowsN, cores) if cores > 1 else (v1, t1)
    return {"value": round(vN, 1), "unit": "Mpix/s", "cores": cores, "kind": "port",
            "value_1core": round(v1, 1), "scaling_1_to_N": round(vN / v1, 2), "runs": 5, "statistic": "median of 5 timed runs after one untimed run",
            "times_s": tN, "times_s_1core": t1, "host": host,
            "sample": "oracle/pixell_oracle.c reproject of %d (all-core) / %d (1-core) centre output rows x %d "
                      "columns x %d components of the same workload" % (rowsN, rows1, nxo, nc)}


def place_buffers(sh, candidates, dev, keep="first", arena=False):
    """Allocate and fill the resident maps.  Where the driver puts a 20 GB buffer physically moves this
    HBM-bound kernel by up to 10 % (profiles/README.md: same virtual addresses, re-allocated, 7.35-8.13 ms).
    The headline number comes from the FIRST allocation, made by one fixed policy: pj.place_pair (class-aware: destination
    across a boundary between two memory classes, found by a topology probe), or with --arena DecStripReprojector.alloc_pair (one
    plain allocation, destination above the source), or --two-allocations.  With
    --placements N > 1 the other N - 1 allocations are only probed (4 launches each, outside every timed step) so
    that the line can say where the first one sits in the spread (roofline.frac_first/median/best_placement);
    --keep-placement best restores round 1's behaviour of running the timed steps on the fastest candidate."""
    import random
    rng = random.Random(os.getpid())
    best = None
    tried = []
    ballast = []
    holds = []
    for k in range(max(1, candidates)):
        if arena == "placed":   # one allocation with head-room, its memory classes mapped with the library's store probe, the
            # destination put across a class boundary (pixell.jl_amd/placement.py): topology discovery, no timing of this workload
            try:
                src, dst, pinfo = pj.place_pair(sh.src_tensor_shape(), sh.dst_tensor_shape(), device=dev)
                pinfo.pop("arena")                   # the views keep the allocation alive
            except Exception as e:                   # noqa: BLE001 -- never lose a run to the placement: plain allocation, and say so
                print("bench.py: pj.place_pair failed (%s: %s); plain allocation instead" % (type(e).__name__, str(e)[:200]), file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
                src, dst, hold = sh.alloc_pair()
                pinfo = {"placement": "place_pair FAILED (%s): plain allocation, destination above the source" % type(e).__name__,
                         "allocation_GiB": None, "classes": None, "class_runs_label_from_to_GiB": None, "probe_us_same_class": None,
                         "probe_us_different_classes": None, "src_offset_GiB": None, "dst_offset_GiB": None, "source": None}
        elif arena == "maps":   # DecStripReprojector.alloc_maps(): the library's default policy for a RESIDENT pair -- one allocation of exactly
            # the pair's size, its destination shifted onto a class boundary by a ballast that is returned (placement.place_pair_shifted)
            try:
                src, dst, minfo = sh.alloc_maps()
                holds.append(minfo.pop("arena", None))
            except Exception as e:                   # noqa: BLE001 -- never lose a run to the placement
                print("bench.py: alloc_maps failed (%s: %s); plain pair instead" % (type(e).__name__, str(e)[:200]), file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
                src, dst, hold = sh.alloc_pair()
                holds.append(hold)
                minfo = {"placement": "alloc_maps FAILED (%s): plain pair" % type(e).__name__}
        elif arena == "api":    # what a caller of the drop-in API gets: the source in a plain allocation, the output allocated by the
            # library's default policy (placement.empty_map: two memory classes when a candidate turns up, no head-room kept)
            src = sh.alloc_src()
            dst, ainfo = pj.empty_map(sh.dst_tensor_shape(), device=dev)
        elif arena:       # one allocation, destination above the source (sharding.alloc_pair: a fixed policy, nothing probed)
            src, dst, hold = sh.alloc_pair()
            holds.append(hold)
        else:
            src = sh.alloc_src()
            dst = sh.alloc_dst()
        fill_strip(sh, src, 1234)
        sh.plan.build_tables()
        n = sh.dst_window[1]
        ts = []
        for _ in range(4):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sh.plan.execute_rows(src, dst, 0, n)      # halo rows are zeros here: same traffic, no exchange needed
            b.record()
            torch.cuda.synchronize(dev)
            ts.append(a.elapsed_time(b))
        t = sorted(ts[1:])[1]
        tried.append(round(t, 4))
        if best is None or (keep == "best" and t < best[2]):
            best = (src, dst, t)
        del src, dst
        if arena not in ("placed", "api", "maps"):
            holds.clear()
        if k + 1 < candidates:
            # return the losing blocks to the driver and perturb the heap so the next try lands elsewhere
            ballast.append(torch.empty(int(rng.uniform(0.3, 3.0) * 2**30), dtype=torch.uint8, device=dev))
            if len(ballast) > 2:
                ballast.pop(0)
            torch.cuda.empty_cache()
    del ballast
    torch.cuda.empty_cache()
    alloc_desc = ("one allocation, destination above the source (DecStripReprojector.alloc_pair: fixed policy, nothing probed)" if arena else "two allocations")
    if arena == "placed":
        alloc_desc = {"policy": "pj.place_pair: one allocation with head-room, memory classes mapped with pxl_mem_probe_pair, destination across a class boundary", **pinfo}
    if arena == "maps":
        alloc_desc = {"policy": "DecStripReprojector.alloc_maps(): the library's default for a resident pair -- ONE allocation of exactly the pair's size, the "
                                "destination put across a class boundary by a scout allocation and a ballast that are both returned (placement.place_pair_shifted)", **minfo}
    if arena == "api":
        alloc_desc = {"policy": "the library's default (what pj.reproject / DecStripReprojector.alloc_maps / the Julia HIPArray constructor allocate with): source "
                                "torch.empty, destination pj.empty_map -- class-aware, no head-room kept", **ainfo}
    return best[0], best[1], {"allocation": alloc_desc, "candidates_ms": tried,
                              "chosen_ms": round(best[2], 4), "chosen": keep,
                              "first_ms": tried[0], "median_ms": sorted(tried)[len(tried) // 2], "best_ms": min(tried)}


def load_traffic(workload):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes
    (profiles/traffic_<workload>.json, produced by tools/make_traffic.py); None if not collected."""
    p = os.path.join(ROOT, "profiles", "traffic_%s.json" % workload)
    if os.path.exists(p):
        with open(p) as f:
            return json.load(f)["hbm_bytes_per_launch"]
    return None


def measure_traffic(workload, timeout_s=90, kernel="k_reproject_dma", child_env=None, raw=False):
    """HBM bytes per launch of k_reproject_dma measured NOW: two child runs of this script under
    `rocprofv3 --kernel-trace --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` (separate passes, the program directly after `--`, as
    /opt/skills/guides/MI355X_MICROARCH.md prescribes; KiB -> bytes; FETCH_SIZE doubled on gfx950).  The caller has released its
    device memory; the children are ordinary child processes (nothing is exec'ed over this one).  Returns (bytes, detail) or
    (None, reason)."""
    import csv
    import glob
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    if "rocprofiler" in os.environ.get("LD_PRELOAD", "") or any(k.startswith("ROCPROF") for k in os.environ):
        return None, "this run is itself being profiled (rocprofiler is preloaded): no nested counter passes"
    out = {}
    tmp = tempfile.mkdtemp(prefix="pxl_pmc_")
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = [exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                   "--workload", workload, "--steps", "3", "--warmup", "1", "--sustain-seconds", "0", "--no-cpu-baseline", "--no-configs",
                   "--no-traffic"]
            env = dict(os.environ, TMPDIR=tmp)
            env.update(child_env or {})
            try:
                r = subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=timeout_s)
            except subprocess.TimeoutExpired:
                return None, "rocprofv3 --pmc %s did not finish within %d s" % (counter, timeout_s)
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None, "rocprofv3 --pmc %s failed (rc %d): %s" % (counter, r.returncode, (r.stderr or "").strip().splitlines()[-1:] or "")
            vals = sorted(float(row["Counter_Value"]) for row in csv.DictReader(open(files[0])) if kernel in row["Kernel_Name"])
            if not vals:
                return None, "no %s rows in the %s pass" % (kernel, counter)
            out[counter] = (vals[len(vals) // 2], len(vals))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if raw:        # the caller applies the corrections that fit its access pattern
        return None, {"fetch_counter_bytes": out["FETCH_SIZE"][0] * 1024.0, "write_bytes": out["WRITE_SIZE"][0] * 1024.0,
                      "launches_sampled": [out["FETCH_SIZE"][1], out["WRITE_SIZE"][1]]}
    fetch = 2.0 * out["FETCH_SIZE"][0] * 1024.0
    write = out["WRITE_SIZE"][0] * 1024.0
    return fetch + write, {"fetch_bytes_x2": fetch, "write_bytes": write, "launches_sampled": [out["FETCH_SIZE"][1], out["WRITE_SIZE"][1]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default=os.environ.get("PXL_BENCH_WORKLOAD", "cfg4"))
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run everything beyond it: the oracle check of the timed output, the `sustained` "
                         "loop, the CPU baseline, the live traffic passes under rocprofv3, the other configs and the evaluators.  "
                         "Without it a run sets up, warms up, times the K steps, writes --dump-outputs and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float64; a fixed, "
                         "seeded sample of rows and values of the output, at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--sustain-seconds", type=float, default=float(os.environ.get("PXL_BENCH_SUSTAIN_S", "5")),
                    help="with --full, after the K timed steps (N = 1): keep issuing steps back to back for this long and report "
                         "their mean as `sustained` (a thermally settled number, and GPU activity an outside sampler can see); 0 = off")
    ap.add_argument("--placements", type=int, default=int(os.environ.get("PXL_BENCH_PLACEMENTS", "1")),
                    help="buffer placements probed at setup (default 1: just the first allocation, which is what the "
                         "headline always reports unless --keep-placement best)")
    ap.add_argument("--api-default", dest="arena", action="store_const", const="api",
                    default={"1": True, "0": False, "placed": "placed", "api": "api", "maps": "maps"}.get(os.environ.get("PXL_BENCH_ARENA", "maps"), "maps"),
                    help="the maps as a caller of the drop-in API gets them: the source in a plain torch allocation, the "
                         "destination from the library's default allocation policy (pj.empty_map: a map of 3 GiB or more is looked for across a "
                         "boundary between two memory classes, rejected candidates are held only during the search, nothing but the map stays "
                         "allocated).  The default run reports the 144-GiB-head-room placement (--placed) and the plain one beside it")
    ap.add_argument("--maps", dest="arena", action="store_const", const="maps",
                    help="(the default) the maps from DecStripReprojector.alloc_maps(): one allocation of exactly the pair's size, destination across a class "
                         "boundary, nothing else kept (placement.place_pair_shifted)")
    ap.add_argument("--placed", dest="arena", action="store_const", const="placed",
                    help="class-aware placement of the maps with head-room, pj.place_pair: ONE allocation with 144 GiB of head-room, its three "
                         "memory classes mapped with the library's store probe (pxl_mem_probe_pair, ~100 probes of 0.3 ms), the destination "
                         "put across a class boundary, the source in a class it does not touch.  The reprojection's eight XCD write fronts "
                         "store at 6.8-7.1 TB/s split over two classes and at 5.8-6.0 TB/s inside one, which is where a plain allocation "
                         "normally lies (DESIGN 4.7; history: docs/DESIGN_history_r01-r03.md 9 item 6).  Topology discovery by a fixed rule: nothing about this workload is timed, no "
                         "candidates are compared.  With N > 1 every rank places its own strip pair.  The default run also reports the "
                         "plain first placement of the same workload (configs.*.plain_first_placement)")
    ap.add_argument("--arena", dest="arena", action="store_true",
                    help="plain allocation, nothing probed: source and destination carved out of ONE allocation, destination above the "
                         "source (DecStripReprojector.alloc_pair; the default of round 2: fast for the 45 GB pair in 20 of 24 processes "
                         "because the driver's block boundary at 32 GiB falls into the destination, slow otherwise)")
    ap.add_argument("--two-allocations", dest="arena", action="store_false",
                    help="allocate the source and the destination separately (round 1's and early round 2's default)")
    ap.add_argument("--keep-placement", default="first", choices=["first", "best"],
                    help="which probed placement the timed steps run on (first = unselected headline)")
    ap.add_argument("--check", action="store_true", help="spot-check the output of the last timed step against the oracle, outside "
                                                         "the timed region (always done with --full)")
    ap.add_argument("--halo", default="auto", choices=["auto", "native", "torch", "gloo"],
                    help="halo transport for N > 1 (auto: the library's native RCCL step over torch's communicator, then over "
                         "a communicator made by pxl_comm_init_rank, then torch P2P; each is pre-flighted on every rank, "
                         "primed and checked against the oracle before it is used; gloo = host-staged, only by name)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (the product path); gloo = host-staged halo, only for rehearsing "
                         "the N-rank flow on a box with fewer GPUs than ranks (with PXL_BENCH_SHARE_GPU=1)")
    ap.add_argument("--no-traffic", action="store_true",
                    help="with --full, do not measure roofline.traffic with two rocprofv3 --pmc child passes after the headline (N = 1, "
                         "default workload); the committed profile of the same workload is quoted instead")
    ap.add_argument("--no-configs", action="store_true",
                    help="with --full, skip the side measurements appended after the headline (configs / evaluators blocks "
                         "and the evaluators' CPU baselines)")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        sys.exit(self_launch(args.gpus, sys.argv[1:]))
    if os.environ.get("PXL_BENCH_SHARE_GPU") and args.arena in ("placed", "api", "maps"):
        # rehearsal: several ranks on ONE device.  The class-aware policies hold ballast / head-room while they look for a class
        # boundary, which ranks sharing a device would fight over; a rehearsal checks the flow, not the rate: plain allocations
        args.arena = True

    # stdout carries exactly one JSON line: libraries (RCCL prints a version banner, gloo its connection notes) write
    # to file descriptor 1 behind Python's back, so everything else is sent to stderr from here on
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))
    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X: there is no CPU fallback for the product path")
    pj.load_library()
    # one rank per GPU; PXL_BENCH_SHARE_GPU=1 lets several ranks share a device for rehearsals on a 1-GPU box
    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", local_rank % ndev if os.environ.get("PXL_BENCH_SHARE_GPU") else local_rank)
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            # eager communicator setup on the rank's own device; lazy when ranks share a GPU for a rehearsal (RCCL then
            # refuses the duplicate device at the first exchange, which exercises the transport fallback below)
            share = bool(os.environ.get("PXL_BENCH_SHARE_GPU"))
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=None if share else dev)
        else:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)

    if args.workload == "cfg5":
        result = bench_scattered(args, rank, world, dev)
    else:
        result = bench_reproject(args, rank, world, dev)
    if args.full and world == 1 and args.workload == "cfg4" and not args.no_traffic and "roofline" in result:
        # roofline.traffic measured in THIS run (the maps of the headline are gone by now; nothing else is on the device)
        torch.cuda.empty_cache()
        t0 = time.perf_counter()
        tb, detail = measure_traffic(args.workload)
        if tb is not None:
            result["roofline"]["traffic"] = tb
            result["roofline"]["traffic_source"] = ("measured in this run: two child passes of this script under rocprofv3 --kernel-trace --pmc "
                                                    "FETCH_SIZE / --pmc WRITE_SIZE (separate passes; KiB -> bytes; FETCH_SIZE x2 on gfx950), median "
                                                    "over the k_reproject_dma launches; %.0f s" % (time.perf_counter() - t0))
            result["roofline"]["traffic_detail"] = detail
        else:
            result["roofline"]["traffic_source"] = (result["roofline"].get("traffic_source") or "") + "; live measurement failed: %s" % detail
    if args.full and world == 1 and args.workload == "cfg4" and not args.no_configs:
        side_measurements(args, dev, result)
    if args.full and world > 1 and args.workload == "cfg4" and not args.no_configs:
        # the other multi-GPU BASELINE config in the same line, after the headline and outside its timed region: cfg5 -- the map
        # replicated on every rank, the 1e9 points split evenly (pj.strip_bounds; rank r generates points [lo, hi) of the one seeded
        # sequence), no data-path collective; same barrier + max-over-ranks timing, every rank's points oracle-checked
        a = argparse.Namespace(**vars(args))
        a.workload, a.steps, a.warmup, a.dump_outputs = "cfg5", 6, 2, None
        torch.cuda.empty_cache()
        r = bench_scattered(a, rank, world, dev)
        result.setdefault("configs", {})["cfg5"] = scattered_record(r, a.steps)
    if rank == 0:
        json_out.write(json.dumps(result) + "\n")
        json_out.flush()
    if world > 1:
        dist.barrier(group=_CTRL)
        dist.destroy_process_group()
    if args.backend == "nccl" and _CTRL is not None and args.halo != "gloo":
        sys.exit(4)                                      # cannot happen (gloo is opt-in); belt and braces


def self_launch(ngpus, argv):
    """`python bench.py --gpus N` from a bare shell (no WORLD_SIZE): start the N ranks as a CHILD job -- this process has
    not touched the GPU and never does; nothing is re-exec'ed -- relay the ranks' one JSON line to stdout, everything
    else to stderr, and return the job's exit code."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ngpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    print("bench.py: no WORLD_SIZE in the environment; starting %d ranks: %s" % (ngpus, " ".join(cmd)), file=sys.stderr, flush=True)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    for line in proc.stdout:
        if line.lstrip().startswith("{"):
            sys.stdout.write(line)
            sys.stdout.flush()
        else:
            sys.stderr.write(line)
    return proc.wait()


_CTRL = None        # gloo control group, set when the RCCL transport failed and the run fell back to gloo


def _on_host():
    """Collectives of the measurement harness run on the host when the job's backend is gloo (rehearsal or fallback)."""
    return _CTRL is not None or dist.get_backend() != "nccl"


def timed_region(world, dev, steps, body):
    if world > 1:
        dist.barrier(group=_CTRL)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for k in range(steps):
        body(k)
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier(group=_CTRL)
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if _on_host() else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=_CTRL)
        dt = float(t.item())
    return dt


def bench_reproject(args, rank, world, dev):
    global _CTRL
    shape_in, wcs_in, shape_out, wcs_out, desc = workload_geometry(args.workload)
    nx, ny, nc = shape_in
    nxo, nyo = shape_out
    sh = pj.DecStripReprojector(shape_in, wcs_in, shape_out, wcs_out, rank, world, dev)
    if args.arena in ("placed", "api", "maps") and args.placements > 1:
        print("bench.py: --placements %d is ignored with the %s allocation policy (one fixed rule, first and only allocation)" % (args.placements, args.arena), file=sys.stderr, flush=True)
    src, dst, placement = place_buffers(sh, 1 if args.arena in ("placed", "api", "maps") else args.placements, dev, args.keep_placement, arena=args.arena)
    torch.cuda.synchronize(dev)
    # ---- choose the halo transport (N > 1).  Candidates in order: "native" = the library's own sharded step (RCCL
    # send/recv issued from C straight out of / into the resident buffer), "torch" = torch.distributed
    # batch_isend_irecv over the same RCCL communicator with packed staging buffers, "gloo" = host-staged (rehearsals
    # and last resort).  The development boxes have one GPU, so the RCCL transports first meet real peers in the
    # driver's multi-GPU run: each candidate is primed (communicator setup is not part of any step) AND its result
    # spot-checked against the oracle on every rank; if any rank raises or mismatches, all ranks agree over a gloo
    # control group to move on to the next candidate.  The JSON line names the transport that ran.
    transport, halo = "none (one rank)", "torch"
    own_comm = None
    if world > 1:
        # gloo is never an N-GPU result: under --backend nccl it is tried only when asked for by name (--halo gloo)
        wanted = {"auto": ["native", "native_own_comm", "torch"], "native": ["native"], "torch": ["torch"], "gloo": ["gloo"]}[args.halo]
        if dist.get_backend() != "nccl":
            wanted, ctrl = ["gloo"], None
        else:
            ctrl = dist.new_group(backend="gloo")

        def agree(flag):
            """MAX over ranks of a 0/1 flag, over the host control group (never over the transport under test)."""
            t = torch.tensor([1 if flag else 0], dtype=torch.int32)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=ctrl)
            return bool(int(t.item()))

        notes = []
        chosen = None
        for cand in wanted:
            err = ""
            # ---- pre-flight: every rank checks locally that it CAN post, and all ranks agree, before anyone posts a
            # send or a receive (a rank that raised before posting would leave its peers waiting for ever)
            try:
                if cand == "native":
                    ok, why = sh.native_ready()
                    if not ok:
                        err = "pre-flight: " + why
                elif cand == "native_own_comm":
                    own_comm = sh.make_own_comm(ctrl)           # collective over the control group + ncclCommInitRank
                elif cand == "gloo" and ctrl is not None:
                    sh.group, sh._staging = ctrl, None
            except Exception as e:                              # noqa: BLE001 -- reported, never swallowed
                err = "pre-flight %s: %s" % (type(e).__name__, (str(e).splitlines() or [""])[0][:200])
            if agree(bool(err)):
                notes.append("%s skipped (%s)" % (cand, err or "pre-flight failed on another rank"))
                print("bench.py rank %d: halo transport %s" % (rank, notes[-1]), file=sys.stderr, flush=True)
                continue
            # ---- prime the transport and check the strip against the oracle; a rank that hangs is a hard failure
            try:
                dst.fill_(float("nan"))
                if cand == "native":
                    sh.step_native(src, dst)
                elif cand == "native_own_comm":
                    sh.step_native(src, dst, comm_ptr=own_comm)
                else:
                    sh.step(src, dst)
                sync_or_die(dev, 120.0, "halo transport %s" % cand)
                chk = spot_check(sh, src, dst, shape_in, wcs_in, shape_out, wcs_out)
                if not chk["bit_identical"]:
                    err = "result differs from the oracle (max abs err %.3g)" % chk["max_abs_err"]
            except Exception as e:                              # noqa: BLE001
                err = "%s: %s" % (type(e).__name__, (str(e).splitlines() or [""])[0][:200])
            if not agree(bool(err)):
                chosen = cand
                break
            notes.append("%s failed (%s)" % (cand, err or "on another rank"))
            print("bench.py rank %d: halo transport %s" % (rank, notes[-1]), file=sys.stderr, flush=True)
        if chosen is None:
            sys.exit("bench.py: no halo transport worked (a host-staged gloo run is not an N-GPU result; ask for it by "
                     "name with --halo gloo): " + "; ".join(notes))
        halo = chosen
        if own_comm is not None and chosen != "native_own_comm":
            sh.close_own_comm()                          # made during a pre-flight, not the transport that runs
            own_comm = None
        if chosen == "gloo" and ctrl is not None:
            _CTRL = ctrl                                 # the harness collectives move to the host as well
        transport = {"native": "RCCL send/recv issued by pxl_reproject_sharded_step over torch's communicator (no staging)",
                     "native_own_comm": "RCCL send/recv issued by pxl_reproject_sharded_step over a communicator made by "
                                        "pxl_comm_init_rank (no staging, no torch in the data path)",
                     "torch": "RCCL via torch.distributed batch_isend_irecv (packed staging buffers)",
                     "gloo": "gloo (host-staged %s) -- NOT an N-GPU result" % ("REHEARSAL" if ctrl is None else "by request")}[chosen]
        if notes:
            transport += "; " + "; ".join(notes)
        dist.barrier(group=_CTRL if _CTRL is not None else ctrl)

    def one_step(k=None, events=None):
        if halo in ("native", "native_own_comm"):
            if events:
                events[0].record()
            sh.step_native(src, dst, comm_ptr=own_comm if halo == "native_own_comm" else None)
            if events:
                events[1].record()
        else:
            sh.step(src, dst, events=events)

    for _ in range(args.warmup):
        one_step()
    torch.cuda.synchronize(dev)

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    dt = timed_region(world, dev, args.steps, lambda k: one_step(k, ev[k]))
    if getattr(args, "dump_outputs", None):
        dump_reproject(args.dump_outputs, dst, sh, (nc, nyo, nxo), rank, world)

    out_values = nxo * nyo * nc
    mpix = out_values * args.steps / dt / 1e6
    # dominant kernel (k_reproject_staged): the launch bracketed by the events
    kms = sorted(a.elapsed_time(b) for a, b in ev)
    k_avg_ms = sum(kms) / len(kms)
    if world == 1:
        launch_out_rows, launch_src_rows = nyo, ny
    elif halo in ("native", "native_own_comm"):  # the events bracket the whole sharded step of this rank
        launch_out_rows, launch_src_rows = sh.dst_window[1], sh.src_window[1]
    elif sh.interior[1] > sh.interior[0]:
        launch_out_rows = sh.interior[1] - sh.interior[0]
        launch_src_rows = sh.own[rank][1] - sh.own[rank][0]
    else:
        launch_out_rows, launch_src_rows = sh.dst_window[1], sh.src_window[1]
    # algorithmic bytes of that launch: source rows read once + output rows written once
    alg_bytes = 8.0 * nc * (launch_src_rows * nx + launch_out_rows * nxo)
    achieved = alg_bytes / (k_avg_ms * 1e-3) / 1e9
    traffic = load_traffic(args.workload) if world == 1 else None

    result = {
        "metric": baseline_metric(),
        "value": round(mpix, 1), "unit": "Mpix/s",
        "value_counts": "output map values per second = sky pixels x %d components (SURVEY 8(d))" % nc,
        "sky_Mpix_s": round(mpix / nc, 1),
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 4),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": desc, "shape_in": list(shape_in), "shape_out": list(shape_out) + [nc],
                   "parallelism": "dec-strip x%d, %d-row halo via %s" % (
                       world, max([hi - lo for _, lo, hi in sh.recvs + sh.sends], default=0),
                       transport),
                   "halo_bytes_per_message": max([(hi - lo) * nx * nc * 8 for _, lo, hi in sh.recvs + sh.sends], default=0),
                   "bytes_per_output_value": round(8.0 * (nx * ny + nxo * nyo) / (nxo * nyo), 3),
                   "buffer_placement": placement},
        "roofline": {"bound": "hbm",
                     "kernel": "k_reproject_dma" + (" (whole sharded step: exchange wait + interior + boundary launches)" if halo in ("native", "native_own_comm") and world > 1 else ""),
                     "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 4),
                     "traffic": traffic,
                     "traffic_source": ("committed rocprofv3 PMC passes of this workload (profiles/traffic_%s.json: FETCH_SIZE x2 + "
                                        "WRITE_SIZE, separate passes); not re-measured in this run" % args.workload) if traffic else None,
                     "algorithmic_bytes_per_launch": alg_bytes,
                     "kernel_ms_avg": round(k_avg_ms, 4), "kernel_ms_min": round(kms[0], 4),
                     "kernel_ms_median": round(kms[len(kms) // 2], 4)},
    }
    full = getattr(args, "full", True)
    if full and world == 1 and args.sustain_seconds > 0:
        # NOT the headline: the K timed steps above are.  A few seconds of the same step, back to back.
        nsus = max(args.steps, int(args.sustain_seconds / (dt / args.steps)))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(nsus):
            one_step()
        b.record()
        torch.cuda.synchronize(dev)
        sus_ms = a.elapsed_time(b) / nsus
        result["sustained"] = {"steps": nsus, "seconds": round(a.elapsed_time(b) / 1e3, 2), "ms_per_step": round(sus_ms, 4),
                               "frac": round(alg_bytes / (sus_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                               "note": "step = table build + reprojection, HIP events around the whole run; not the headline"}
    if world == 1 and args.placements > 1:
        # where the timed placement sits among the probed ones (probe medians of 4 launches each)
        f = lambda ms: round(alg_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
        result["roofline"].update({"frac_first_placement": f(placement["first_ms"]),
                                   "frac_median_placement": f(placement["median_ms"]),
                                   "frac_best_placement": f(placement["best_ms"])})
    if full or args.check:
        # the output of the LAST timed step is verified (outside the timed region): every rank checks rows of its own
        # strip (row 0 of a strip is the one that needs the halo) against the oracle; the worst case is reported
        result["check"] = reduce_check(spot_check(sh, src, dst, shape_in, wcs_in, shape_out, wcs_out), world, dev)
    if own_comm is not None:
        torch.cuda.synchronize(dev)
        sh.close_own_comm()
    if full and world == 1 and rank == 0 and not args.no_cpu_baseline:
        del src, dst
        torch.cuda.empty_cache()
        result["cpu_baseline"] = cpu_baseline_reproject(shape_in, wcs_in, shape_out, wcs_out)
    return result


def sync_or_die(dev, seconds, what):
    """torch.cuda.synchronize with a deadline: a receive that is never matched would otherwise hang the rank (and
    the job) for ever.  On timeout the process exits non-zero at once -- the launcher then takes the job down."""
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    t0 = time.perf_counter()
    while not ev.query():
        if time.perf_counter() - t0 > seconds:
            print("bench.py: %s did not complete within %.0f s on this rank; aborting the job" % (what, seconds),
                  file=sys.stderr, flush=True)
            os._exit(3)
        time.sleep(0.002)
    torch.cuda.synchronize(dev)


def spot_check(sh, src, dst, shape_in, wcs_in, shape_out, wcs_out, nrows=6):
    """Compare a few output rows of this rank's strip with the oracle fed the same source rows."""
    import numpy as np
    from oracle import oracle as O
    lo, n = sh.dst_window
    worst = 0.0
    bit_identical = True
    for r in sorted({0, n // 3, n // 2, n - 1}):
        s_lo, s_hi = O.reproject_src_rows(wcs_in, shape_in, wcs_out, shape_out, lo + r, 1)
        s = src[:, s_lo - sh.buf_lo:s_hi - sh.buf_lo, :].cpu().numpy()
        exp = O.reproject(wcs_in, shape_in, s, wcs_out, shape_out, src_row0=s_lo, src_nrows=s_hi - s_lo,
                          dst_row0=lo + r, dst_nrows=1)
        got = dst[:, r:r + 1, :].cpu().numpy()
        worst = max(worst, float(np.abs(got - exp).max()))
        bit_identical &= bool(np.array_equal(got.view(np.int64), exp.view(np.int64)))
    return {"max_abs_err": worst, "bit_identical": bit_identical}


def reduce_check(chk, world, dev):
    """Every rank checks its own strip / its own points against the oracle; the job reports the WORST case: the largest error
    of any rank, bit-identical only if every rank was, and how many ranks took part (MAX over the job's ranks, on the host when
    the control plane is gloo)."""
    if world == 1:
        return chk
    where = "cpu" if _on_host() else dev
    t = torch.tensor([chk["max_abs_err"], 0.0 if chk["bit_identical"] else 1.0], dtype=torch.float64, device=where)
    cnt = torch.ones(1, dtype=torch.float64, device=where)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=_CTRL)
    dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=_CTRL)
    out = dict(chk)
    out.update({"max_abs_err": float(t[0]), "bit_identical": bool(t[1] == 0.0), "ranks_checked": int(round(float(cnt[0])))})
    return out


DUMP_SEED = 20251016             # --dump-outputs: the sampled indices depend on this and on the workload's shape only
DUMP_VALUES = 1 << 20            # single values sampled over the whole output (8 MB, and 8 MB of their indices)
DUMP_ROW_BYTES = 32 << 20        # whole output rows: at most 16 of them and at most this many bytes


def _sample_index(total, k):
    """Sorted distinct flat indices in [0, total), the same for every run of the same workload."""
    import numpy as np
    return np.unique(np.random.default_rng(DUMP_SEED).integers(0, total, size=min(k, total), dtype=np.int64))


def _gather_rank0(obj, world):
    """Every rank's object in rank order on rank 0, None on the other ranks."""
    if world == 1:
        return [obj]
    got = [None] * world if dist.get_rank() == 0 else None
    dist.gather_object(obj, got, dst=0, group=_CTRL)
    return got


def _write_dump(dirname, arrays):
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def dump_reproject(dirname, dst, sh, shape, rank, world):
    """--dump-outputs of a reprojection workload: the output map (components, rows, columns) as the last timed step left it, as a
    fixed sample -- whole rows spread evenly from the first to the last (output_rows at output_row_index) and seeded single values
    over the whole map (output_sample at the flat indices output_sample_index).  Every rank reads its own strip, rank 0 writes."""
    import numpy as np
    nc, nyo, nxo = shape
    lo, n = sh.dst_window
    krows = max(1, min(16, nyo, DUMP_ROW_BYTES // (8 * nc * nxo)))
    rows = np.unique(np.linspace(0, nyo - 1, krows).round().astype(np.int64))
    mine = rows[(rows >= lo) & (rows < lo + n)]
    part_rows = dst[:, torch.from_numpy(mine - lo).to(dst.device), :].cpu().numpy()
    flat = _sample_index(nc * nyo * nxo, DUMP_VALUES)
    c, rem = np.divmod(flat, nyo * nxo)
    r, x = np.divmod(rem, nxo)
    sel = (r >= lo) & (r < lo + n)
    part_vals = dst[torch.from_numpy(c[sel]).to(dst.device), torch.from_numpy(r[sel] - lo).to(dst.device),
                    torch.from_numpy(x[sel]).to(dst.device)].cpu().numpy()
    parts = _gather_rank0((mine, part_rows, sel, part_vals), world)
    if rank != 0:
        return
    vals = np.empty(flat.size)
    for _, _, s, v in parts:
        vals[s] = v
    _write_dump(dirname, {"output_rows": np.concatenate([p[1] for p in parts], axis=1),
                          "output_row_index": np.concatenate([p[0] for p in parts]),
                          "output_sample": vals, "output_sample_index": flat})


def dump_scattered(dirname, out, lo, total, world):
    """--dump-outputs of cfg5: the sampled value of every point is the output; seeded points over the whole batch (output_sample
    at the point indices output_sample_index).  Every rank reads its own points, rank 0 writes."""
    import numpy as np
    n = out.shape[1]
    flat = _sample_index(total, DUMP_VALUES)
    sel = (flat >= lo) & (flat < lo + n)
    part = out[0, torch.from_numpy(flat[sel] - lo).to(out.device)].cpu().numpy()
    parts = _gather_rank0((sel, part), world)
    if parts is None:
        return
    vals = np.empty(flat.size)
    for s, v in parts:
        vals[s] = v
    _write_dump(dirname, {"output_sample": vals, "output_sample_index": flat})


def scattered_record(r, steps):
    """The compact `configs.cfg5` record of a bench_scattered result."""
    return {"workload": r["config"]["workload"], "parallelism": r["config"]["parallelism"], "Mpts_s": r["value"], "ms_per_step": r["ms_per_step"],
            "n_gpus": r["n_gpus"], "scaling": r["scaling"], "kernel": r["roofline"]["kernel"], "kernel_ms_avg": r["roofline"]["kernel_ms_avg"],
            "frac": r["roofline"]["frac"], "traffic": r["roofline"].get("traffic"), "steps": steps, "sampler": r["config"]["sampler"],
            "check": r["check"], "variants": r.get("variants")}


def bench_scattered(args, rank, world, dev):
    npts_total = int(float(os.environ.get("PXL_BENCH_POINTS", "1e9")))
    shape, wcs = pj.fullsky_geometry(2 * math.pi / 43200)
    nx, ny = shape
    lo, hi = pj.strip_bounds(npts_total, world, rank)
    n = hi - lo
    m = pj.Enmap(torch.empty((ny, nx), dtype=torch.float64, device=dev), wcs)
    pj.fill_random_(m.data, 1234, 0, "normal")                      # replicated map
    sky = torch.empty((n, 2), dtype=torch.float64, device=dev)
    pj.fill_sphere_points_(sky, 42, offset=lo)                      # uniform on the sphere, seed 42
    out = torch.empty((1, n), dtype=torch.float64, device=dev)
    lib = pj.load_library()
    import ctypes as C
    wref = wcs.to_struct()
    shp = pj._lib.shape_arr((nx, ny, 1))

    # PXL_BENCH_SAMPLER=pairs (default when a rank has >= 3e8 points): every step re-lays the map into sector-grouped row
    # pairs (one streaming pass, inside the timed step) and samples from that copy -- 1.0 instead of ~2.25 random sectors
    # per point; "direct" = 4 taps straight from the Julia-layout map.  Both give the same bits.
    mode = os.environ.get("PXL_BENCH_SAMPLER", "auto")
    if mode == "auto":      # the per-step re-layout (~5 ms, constant per rank; 23 ps saved per point) only pays on a large batch
        mode = "pairs" if n >= 3e8 else "direct"
    pairs = torch.empty(lib.pxl_sample_pairs_elems(shp, ny), dtype=torch.float64, device=dev) if mode == "pairs" else None

    def step(k, ev=None, how=mode, rebuild=True):
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if how == "pairs" and rebuild:
            pj._lib.check(lib.pxl_sample_build_pairs_f64(shp, C.c_void_p(m.data.data_ptr()), ny, C.c_void_p(pairs.data_ptr()), s))
        if ev:
            ev[0].record()
        if how == "pairs":
            pj._lib.check(lib.pxl_sample_car_bilinear_pairs_f64(C.byref(wref), shp, C.c_void_p(pairs.data_ptr()), 0, ny, n,
                                                                C.c_void_p(sky.data_ptr()), C.c_void_p(out.data_ptr()), s))
        else:
            pj._lib.check(lib.pxl_sample_car_bilinear_f64(C.byref(wref), shp, C.c_void_p(m.data.data_ptr()), 0, ny, n,
                                                          C.c_void_p(sky.data_ptr()), C.c_void_p(out.data_ptr()), s))
        if ev:
            ev[1].record()

    for k in range(args.warmup):
        step(k)
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    dt = timed_region(world, dev, args.steps, lambda k: step(k, ev[k]))
    if getattr(args, "dump_outputs", None):
        dump_scattered(args.dump_outputs, out, lo, npts_total, world)
    kms = sorted(a.elapsed_time(b) for a, b in ev)
    k_avg_ms = sum(kms) / len(kms)
    alg = 56.0 * n                                                  # 16 coords + 4x8 taps + 8 out
    achieved = alg / (k_avg_ms * 1e-3) / 1e9
    result = {
        "metric": "Mpts/s scattered sky2pix + bilinear sample (Float64)",
        "value": round(npts_total * args.steps / dt / 1e6, 1), "unit": "Mpts/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "cfg5: %.3g uniform-on-sphere points sampled from a replicated 43200x21601 map" % npts_total,
                   "parallelism": "replicated map, points sharded x%d, no collective" % world,
                   "sampler": "row-pair copy of the map rebuilt inside every step" if mode == "pairs" else "direct 4-tap gather"},
        "roofline": {"bound": "hbm", "kernel": "k_sample_pairs" if mode == "pairs" else "k_sample_bilinear", "achieved": round(achieved, 1),
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": None,
                     "algorithmic_bytes_per_launch": alg, "sector_granular_bytes_per_launch": 152.0 * n,
                     "kernel_ms_avg": round(k_avg_ms, 4)},
    }
    full = getattr(args, "full", True)
    if full or args.check:
        # the output of the last timed step against the oracle on a seeded subset of this rank's points (outside the timed region)
        result["check"] = scattered_check(m, wcs, shape, sky, out, world, dev)
    if full and world == 1 and mode == "pairs":
        # the two other ways a caller can run the same batch (not the headline; HIP events around each step):
        # the map does NOT change between batches -- the row-pair copy is built once and reused -- and the direct sampler
        def timed(how, rebuild, steps):
            step(0, None, how, rebuild)
            torch.cuda.synchronize(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(steps):
                step(k, None, how, rebuild)
            b.record()
            torch.cuda.synchronize(dev)
            return round(a.elapsed_time(b) / steps, 4)
        fixed_ms = timed("pairs", False, max(3, args.steps))
        fixed_chk = scattered_check(m, wcs, shape, sky, out, world, dev)
        direct_ms = timed("direct", False, max(2, args.steps // 3))
        direct_chk = scattered_check(m, wcs, shape, sky, out, world, dev)
        result["variants"] = {
            "map_changes_every_step": {"ms_per_step": result["ms_per_step"], "note": "the headline: the row-pair copy is rebuilt inside every step"},
            "map_fixed": {"ms_per_step": fixed_ms, "check": fixed_chk,
                          "note": "row-pair copy built once (pj.SamplePairs) and reused: what a caller sampling one map with many batches pays"},
            "direct": {"ms_per_step": direct_ms, "check": direct_chk, "note": "pxl_sample_car_bilinear_f64 straight from the Julia-layout map (no copy)"}}
    return result


def scattered_check(m, wcs, shape, sky, out, world, dev, npick=4096):
    """A seeded subset of this rank's points through the oracle's sampler (same map bytes, same coordinates)."""
    import numpy as np
    from oracle import oracle as O
    n = sky.shape[0]
    g = torch.Generator(device="cpu").manual_seed(7)
    idx = torch.randint(0, n, (min(npick, n),), generator=g).to(dev)
    pts = sky[idx].cpu().numpy()
    got = out[0, idx].cpu().numpy()
    exp = O.sample_bilinear(wcs, (shape[0], shape[1], 1), m.data.cpu().numpy()[None], pts)[0]
    chk = {"points_checked": int(idx.numel()), "max_abs_err": float(np.abs(got - exp).max()),
           "bit_identical": bool(np.array_equal(got.view(np.int64), exp.view(np.int64)))}
    return reduce_check(chk, world, dev)


def side_measurements(args, dev, result):
    """After the headline, outside its timed region (N = 1, default workload): the other BASELINE configs, the
    evaluators the reference has, and the CPU oracle's rates for them -- so that one driver-observed line carries
    what used to live only in builder-kept files under profiles/.  Every reprojection config is measured three ways: through the
    drop-in API with the library allocating the output (api_default: the policy the headline uses too), with the 144-GiB-head-room
    placement (pj.place_pair) and with a plain, unprobed first placement (alloc_pair)."""
    cfgs = {}
    for name in ("cfg2", "cfg3", "cfg3s", "cfg4"):
        a = argparse.Namespace(**vars(args))
        a.workload, a.steps, a.warmup, a.sustain_seconds, a.no_cpu_baseline, a.placements = name, 10, 2, 0.0, True, 1
        a.dump_outputs = None
        if name == "cfg2":
            a.arena = True
            r = variant(a, dev)
            r["note"] = "268 MB of output: Infinity-Cache resident, not roofline evidence (SURVEY 8(d)); plain allocation"
            cfgs[name] = r
            continue
        if name == "cfg4" and args.arena == "placed":       # the headline IS the class-aware run of this config (only with --placed)
            placed = {"Mpix_s": result["value"], "ms_per_step": result["ms_per_step"], "kernel_ms_avg": result["roofline"]["kernel_ms_avg"],
                      "frac": result["roofline"]["frac"], "check": result["check"], "note": "the headline above"}
        else:
            a.arena = "placed"
            placed = variant(a, dev)
        a.arena = True
        plain = variant(a, dev)
        api = api_default_record(name, dev)
        # the record's own numbers are what the drop-in API delivers (api_default); the two other allocation policies beside it
        cfgs[name] = {"workload": plain.pop("workload"), "bytes_per_output_value": plain.pop("bytes_per_output_value"),
                      "kernel_ms_avg": api["ms_per_call"], "frac": api["frac"], "check": api["check"],
                      "numbers_are": "api_default: pj.reproject(m, shape_out, wcs_out) with the library allocating the output",
                      "api_default": api, "class_aware_placement": placed, "plain_first_placement": plain}
        cfgs[name]["class_aware_placement"].pop("workload", None)
        cfgs[name]["class_aware_placement"].pop("bytes_per_output_value", None)
    a = argparse.Namespace(**vars(args))
    a.workload, a.steps, a.warmup, a.dump_outputs = "cfg5", 6, 2, None
    torch.cuda.empty_cache()
    r = bench_scattered(a, 0, 1, dev)
    cfgs["cfg5"] = scattered_record(r, a.steps)
    if not args.no_traffic:
        # config 5's traffic, measured like the headline's (two rocprofv3 --pmc child passes) on 1e8 points of the same map: the
        # taps are random 16-byte pairs inside one 64-byte sector, for which FETCH_SIZE (64 B per fabric request) is EXACT; the
        # coordinate stream is a wide coalesced read that the counter tallies at half (the x2 rule of the guide), so half of
        # its 16 B per point is added back; the 8-B-per-point output stream is written with 8-byte stores (WRITE_SIZE as read)
        torch.cuda.empty_cache()
        npts = 1e8
        _tb, det = measure_traffic("cfg5", timeout_s=120, kernel="k_sample_pairs", raw=True,
                                   child_env={"PXL_BENCH_POINTS": "%g" % npts, "PXL_BENCH_SAMPLER": "pairs"})
        if isinstance(det, dict):
            corrected = det["fetch_counter_bytes"] + 8.0 * npts + det["write_bytes"]
            cfgs["cfg5"]["traffic"] = {"bytes_per_point": round(corrected / npts, 1), "fetch_counter_bytes_per_point": round(det["fetch_counter_bytes"] / npts, 1),
                                       "write_bytes_per_point": round(det["write_bytes"] / npts, 1), "algorithmic_bytes_per_point": 56.0,
                                       "sector_granular_bytes_per_point": 16 + 64 + 8, "points": npts, "launches_sampled": det["launches_sampled"],
                                       "correction": "FETCH_SIZE as read for the random sector reads (exact) + 8 B/point for the coalesced coordinate stream it tallies at half; WRITE_SIZE as read",
                                       "kernel": "k_sample_pairs (the row-pair copy is built outside this kernel: k_build_rowpairs streams the map once per rebuild)"}
        else:
            cfgs["cfg5"]["traffic"] = None
            cfgs["cfg5"]["traffic_note"] = "live measurement failed: %s" % (det,)
    torch.cuda.empty_cache()
    result["configs"] = cfgs
    # the headline's workload under the two other allocation policies, at the top of the roofline block
    if "cfg4" in cfgs and "roofline" in result:
        result["roofline"]["headline_allocation_policy"] = {True: "plain (alloc_pair)", False: "two plain allocations", "placed": "pj.place_pair (144 GiB head-room)", "maps": "DecStripReprojector.alloc_maps (exact pair, destination across a class boundary)",
                                                            "api": "the library's default (pj.empty_map: class-aware, no head-room)"}.get(args.arena, str(args.arena))
        result["roofline"]["frac_other_policies"] = {"class_aware_placement_144GiB_headroom": cfgs["cfg4"]["class_aware_placement"]["frac"],
                                                     "plain_first_placement": cfgs["cfg4"]["plain_first_placement"]["frac"],
                                                     "api_default_through_pj_reproject": cfgs["cfg4"]["api_default"]["frac"]}
    result["evaluators"] = gpu_evaluators(dev)
    torch.cuda.empty_cache()
    if "cpu_baseline" in result:
        result["cpu_baseline"].update(cpu_baseline_evaluators())


def api_default_record(name, dev, steps=10, warmup=2):
    """EXACTLY what a caller of the drop-in API gets: the source map in a plain torch allocation wrapped in an
    Enmap, `out = pj.reproject(m, shape_out, wcs_out)` -- the library allocates the output by its default policy
    (placement.empty_map: class-aware, no head-room kept) --, then the same call repeated with `out=` and `plan=` reused, HIP
    events around each call (table build + reprojection, like a headline step).  Reports the kernel-level time per call, what
    the first call cost (allocation search + plan + tables + launch), the memory held afterwards against the size of the pair,
    and an oracle check of the output."""
    import types
    shape_in, wcs_in, shape_out, wcs_out, desc = workload_geometry(name)
    nx, ny, nc = shape_in
    nxo, nyo = shape_out
    torch.cuda.empty_cache()
    base_reserved = torch.cuda.memory_reserved(dev)
    src = torch.empty((nc, ny, nx), dtype=torch.float64, device=dev)
    for c in range(nc):
        pj.fill_random_(src[c], 1234 + c)
    m = pj.Enmap(src if nc > 1 else src[0], wcs_in)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = pj.reproject(m, shape_out, wcs_out)
    torch.cuda.synchronize(dev)
    first_s = time.perf_counter() - t0
    held = torch.cuda.memory_reserved(dev) - base_reserved
    alloc_info = pj.last_allocation_info()
    pair = 8.0 * nc * (nx * ny + nxo * nyo)
    plan = pj.ReprojectPlan(m.shape, m.wcs, shape_out, wcs_out, device=dev)
    for _ in range(warmup):
        pj.reproject(m, shape_out, wcs_out, out=out, plan=plan)
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        pj.reproject(m, shape_out, wcs_out, out=out, plan=plan)
        b.record()
    torch.cuda.synchronize(dev)
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    avg = sum(ms) / len(ms)
    dst3 = out.data if out.data.dim() == 3 else out.data[None]
    chk = spot_check(types.SimpleNamespace(dst_window=(0, nyo), buf_lo=0), src, dst3, shape_in, wcs_in, shape_out, wcs_out)
    rec = {"call": "pj.reproject(m, shape_out, wcs_out): output allocated by the library (policy %r), source in a plain torch.empty" % pj.allocation_policy(),
           "ms_per_call": round(avg, 4), "ms_median": round(ms[len(ms) // 2], 4), "frac": round(pair / (avg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "Mpix_s": round(nxo * nyo * nc / (avg * 1e-3) / 1e6, 1), "steps": steps,
           "first_call_s": round(first_s, 3), "held_after_call_GiB": round(held / 2**30, 2), "pair_GiB": round(pair / 2**30, 2),
           "held_over_pair": round(held / pair, 3), "allocation": alloc_info, "check": chk}
    plan.close()
    del out, m, src, dst3
    torch.cuda.empty_cache()
    return rec


def variant(a, dev):
    """One reprojection workload with the allocation policy of a.arena, as a compact record."""
    torch.cuda.empty_cache()
    r = bench_reproject(a, 0, 1, dev)
    torch.cuda.empty_cache()
    out = {"workload": r["config"]["workload"], "bytes_per_output_value": r["config"]["bytes_per_output_value"], "Mpix_s": r["value"],
           "ms_per_step": r["ms_per_step"], "kernel_ms_avg": r["roofline"]["kernel_ms_avg"], "frac": r["roofline"]["frac"],
           "steps": a.steps, "check": r["check"]}
    al = r["config"]["buffer_placement"]["allocation"]
    if isinstance(al, dict):
        out.update({"placement": al["placement"], "source": al.get("source"), "allocation_GiB": al["allocation_GiB"], "classes": al["classes"],
                    "class_runs_label_from_to_GiB": al["class_runs_label_from_to_GiB"], "probe_us_same_class": al["probe_us_same_class"],
                    "probe_us_different_classes": al["probe_us_different_classes"]})
    else:
        out["allocation"] = al
    return out


def _median_ms(fn, dev, reps=7):
    fn()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def gpu_evaluators(dev):
    """The reference's own batched functions on the 0.5-arcmin full-sky geometry: posmap (enmap_ops.jl:190-203), pix2sky!
    and sky2pix! on 2xN batches (car_proj.jl:92-122, 165-200); HIP-event medians, bytes as in SURVEY 8(a)."""
    shape, wcs = pj.fullsky_geometry(2 * math.pi / 43200)
    g = (shape, wcs)
    out = {}

    def rec(name, ms, nbytes, units, unit, ref):
        out[name] = {"ms": round(ms, 4), "GBs": round(nbytes / ms / 1e6, 1), "frac": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4),
                     unit: round(units / ms / 1e3, 1), "reference": ref}
    npx = shape[0] * shape[1]
    ra = torch.empty((shape[1], shape[0]), dtype=torch.float64, device=dev)
    dec = torch.empty_like(ra)
    lib = pj.load_library()
    import ctypes as C
    wref = wcs.to_struct()
    sh2 = (C.c_int64 * 2)(shape[0], shape[1])

    def posmap():
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        pj._lib.check(lib.pxl_posmap_car_f64(C.byref(wref), sh2, 0, shape[1], C.c_void_p(ra.data_ptr()), C.c_void_p(dec.data_ptr()), 1, s))
    rec("posmap", _median_ms(posmap, dev), 16.0 * npx, npx, "Mpix_s", "enmap_ops.jl:190-203 (safe=true), 43200x21601, write-only 16 B/pixel; two plain allocations")
    del ra, dec
    torch.cuda.empty_cache()
    try:    # the same launch with its two output maps in different memory classes (pj.place_streams)
        (ra, dec), sinfo = pj.place_streams([(shape[1], shape[0])] * 2, device=dev)
        rec("posmap, RA and DEC maps in different memory classes", _median_ms(posmap, dev), 16.0 * npx, npx, "Mpix_s",
            "the same launch; buffers from pj.place_streams: classes %s" % [b["class"] for b in sinfo["buffers"]])
        del ra, dec, sinfo
    except Exception as e:                                  # noqa: BLE001 -- a side measurement: reported, not fatal
        out["posmap, RA and DEC maps in different memory classes"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    torch.cuda.empty_cache()
    n = 200_000_000
    pix = torch.empty((n, 2), dtype=torch.float64, device=dev)
    pj.fill_random_(pix, 1, kind="uniform")
    pix.mul_(float(shape[1]))
    sky = torch.empty_like(pix)
    rec("pix2sky!(safe=false)", _median_ms(lambda: pj.pix2sky_(g, pix, sky, safe=False), dev), 32.0 * n, n, "Mpts_s", "car_proj.jl:92-122, 2xN, 2e8 points")
    back = torch.empty_like(pix)
    rec("sky2pix!(safe=true)", _median_ms(lambda: pj.sky2pix_(g, sky, back, safe=True), dev), 32.0 * n, n, "Mpts_s", "car_proj.jl:165-200, 2xN, 2e8 points")
    del back
    nb = n // 2
    rec("pix2sky!(safe=true)", _median_ms(lambda: pj.pix2sky_(g, pix[:nb], sky[:nb], safe=True), dev, reps=5), 32.0 * nb, nb, "Mpts_s",
        "car_proj.jl:92-122 with unwind! (enmap_ops.jl:26-32), 2xN, 1e8 points")
    del pix, sky
    torch.cuda.empty_cache()
    # the Gnomonic evaluators (tan_proj.jl:44-75: two N-vectors in, two out) and the Gnomonic posmap of an 8192^2 patch of 0.5' pixels
    N = 8192
    tan = pj.Gnomonic((-0.5 / 60, 0.5 / 60), (N / 2 + 0.5, N / 2 + 0.5), (40.0, -25.0))
    tg = ((N, N), tan)
    nt = 100_000_000
    ip = torch.empty(nt, dtype=torch.float64, device=dev).uniform_(1.0, float(N))
    jp = torch.empty(nt, dtype=torch.float64, device=dev).uniform_(1.0, float(N))
    tra, tdec = pj.pix2sky(tg, ip, jp, safe=False)
    rec("Gnomonic pix2sky(i, j)", _median_ms(lambda: pj.pix2sky(tg, ip, jp, safe=False), dev, reps=5), 32.0 * nt, nt, "Mpts_s",
        "tan_proj.jl:59-75, two N-vectors, 1e8 points, FP64-transcendental bound (pxl_fastmath.h)")
    rec("Gnomonic sky2pix(ra, dec)", _median_ms(lambda: pj.sky2pix(tg, tra, tdec, safe=False), dev, reps=5), 32.0 * nt, nt, "Mpts_s",
        "tan_proj.jl:44-57, two N-vectors, 1e8 points")
    rec("Gnomonic posmap 8192^2", _median_ms(lambda: pj.posmap((N, N), tan, device=dev), dev, reps=5), 16.0 * N * N, N * N, "Mpix_s",
        "enmap_ops.jl:190-203 on a Gnomonic WCS, write-only 16 B/pixel")
    del ip, jp, tra, tdec
    torch.cuda.empty_cache()
    try:
        out["CAR->TAN mosaic"] = tan_mosaic_record(dev)
    except Exception as e:                                  # noqa: BLE001 -- a side measurement: reported, not fatal
        out["CAR->TAN mosaic"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    torch.cuda.empty_cache()
    return out


def tan_mosaic_record(dev, npatch=4096):
    """SURVEY 8(f) N2 at scale: the full-sky 0.5-arcmin CAR map (7.5 GB) reprojected onto a mosaic of sixteen
    Gnomonic patches of 4096^2 pixels of 0.5 arcmin (2.1 GB of output, far beyond the Infinity Cache), one pj.reproject call per
    patch.  Algorithmic bytes = 8 B written + 8 B read per output pixel (the patches have the source's resolution).  A 128 x 64
    window of the last patch is checked against the oracle's per-pixel evaluation (reference evaluators + libm) of the SAME
    window geometry: the tiled kernel interpolates the coordinates within 1e-10 pixel, i.e. ~2e-10 in value on a white-noise map."""
    import numpy as np
    from oracle import oracle as O
    shape, wcs = pj.fullsky_geometry(2 * math.pi / 43200)
    m = pj.Enmap(torch.empty((shape[1], shape[0]), dtype=torch.float64, device=dev), wcs)
    pj.fill_random_(m.data, 1234)
    res = 0.5 / 60
    patches = [pj.Gnomonic((res, res), (npatch / 2 + 0.5, npatch / 2 + 0.5), (float(ra), dec)) for dec in (-25.0, 25.0) for ra in range(0, 360, 45)]
    outs = [None]

    def run_one_shot():
        outs[0] = [pj.reproject(m, (npatch, npatch), w) for w in patches]
    ms_one_shot = _median_ms(run_one_shot, dev, reps=3)
    one_shot_last = outs[0][-1].data.clone()
    # the record's own numbers: one GenericReprojectPlan per patch (its coordinate lattice and per-pixel tile list, made once and
    # outside the timed region -- exactly what ReprojectPlan's tables are to the CAR -> CAR configs above), outputs allocated once
    plans = [pj.GenericReprojectPlan(shape, wcs, (npatch, npatch), w, device=dev) for w in patches]
    outs[0] = [pj.Enmap(torch.empty((npatch, npatch), dtype=torch.float64, device=dev), w) for w in patches]

    def run():
        for o, pl in zip(outs[0], plans):
            pl.execute(m.data, o.data)                      # = pj.reproject(m, shape, w, out=o, plan=pl) less its argument checks
    ms = _median_ms(run, dev, reps=3)
    same_bits = bool((outs[0][-1].data.view(torch.int64) == one_shot_last.view(torch.int64)).all().item())
    del one_shot_last
    npix = len(patches) * npatch * npatch
    alg = 16.0 * npix
    # the check: a window of the last patch, as its own (shifted-crpix) Gnomonic geometry, through the oracle
    w = patches[-1]
    c0, r0, cw, rw = 1000, 3000, 128, 64
    wwin = pj.Gnomonic(w.cdelt, (w.crpix[0] - c0, w.crpix[1] - r0), w.crval)
    src_host = m.data.cpu().numpy()[None]
    exp = O.reproject_generic(wcs, 0, (shape[0], shape[1], 1), src_host, wwin, 1, (cw, rw))[0]
    got = outs[0][-1].data[r0:r0 + rw, c0:c0 + cw].cpu().numpy()
    err = float(np.abs(got - exp).max())
    ex, tot = plans[-1].tiles()
    return {"ms": round(ms, 4), "GBs": round(alg / ms / 1e6, 1), "frac": round(alg / ms / 1e6 / HBM_PEAK_GBS, 4), "Gpix_s": round(npix / ms / 1e6, 1),
            "patches": len(patches), "patch": [npatch, npatch], "algorithmic_bytes": alg,
            "numbers_are": "plans reused: GenericReprojectPlan.execute(src, dst) per patch (what pj.reproject(m, shape, wcs_patch, out=, plan=) calls) -- the pixel kernel alone",
            "kernels": "k_reproject_generic_tiled3 per patch (k_generic_lattice once per plan; k_reproject_generic_exact_tiles only for plans with per-pixel tiles)",
            "one_shot": {"ms": round(ms_one_shot, 4), "frac": round(alg / ms_one_shot / 1e6 / HBM_PEAK_GBS, 4),
                         "what": "pj.reproject(m, shape, wcs_patch) per patch: lattice + pixels + per-pixel-tiles launch + output allocation every call",
                         "bit_identical_to_plans": same_bits},
            "last_patch_exact_tiles": [ex, tot],
            "check": {"max_abs_err_vs_oracle": err, "window": [cw, rw], "within_2e-9": bool(err < 2e-9)},
            "reference": "pix2sky(out; tan_proj.jl:59-75) -> sky2pix(in; car_proj.jl:225-231, safe=true) -> 2x2 gather, coordinates interpolated per 128x32 tile with a 1e-10-pixel check"}


def cpu_baseline_evaluators():
    """The oracle's loops for the functions the reference DOES have (posmap: enmap_ops.jl:190-203; pix2sky! / sky2pix! on
    2xN: car_proj.jl:92-122, 165-200, safe=true as the reference defaults), on bounded samples of the 0.5-arcmin geometry:
    one core (the reference's execution model) and every CPU this process may use (OpenMP), median of 5 runs each into
    outputs that exist and have been touched before the first timed run."""
    import numpy as np
    from oracle import oracle as O
    shape, wcs = pj.fullsky_geometry(2 * math.pi / 43200)
    nx, ny = shape
    host = host_cpu_share()
    cores = max(1, min(O.max_threads(), host["threads"]))
    res = {}

    def posmap_leg(nrows, threads):
        out = (np.empty((nrows, nx)), np.empty((nrows, nx)))
        rate, times = _cpu_median_rate(lambda: O.posmap(wcs, shape, row0=ny // 2 - nrows // 2, nrows=nrows, out=out), nx * nrows, threads)
        return rate / 1e6, times
    rows1 = 2400                                       # ~0.5 s on one core at ~200 Mpix/s
    v1, t1 = posmap_leg(rows1, 1)
    vcal, _ = posmap_leg(rows1, cores) if cores > 1 else (v1, None)
    rowsN = int(max(rows1, min(0.7 * vcal * 1e6 / nx, 8000)))
    vN, tN = posmap_leg(rowsN, cores) if cores > 1 else (v1, t1)
    res["posmap"] = {"value": round(vN, 1), "value_1core": round(v1, 1), "scaling_1_to_N": round(vN / v1, 2), "unit": "Mpix/s", "cores": cores,
                     "kind": "port", "runs": 5, "times_s": tN, "times_s_1core": t1,
                     "sample": "oracle posmap (enmap_ops.jl:190-203, safe=true) of %d (all-core) / %d (1-core) centre rows x %d columns" % (rowsN, rows1, nx)}
    rng = np.random.default_rng(1)
    n1 = 20_000_000
    nN = int(min(200_000_000, max(n1, n1 * cores // 2)))
    pix = rng.random((nN, 2)) * ny
    O.set_threads(cores)
    sky_pts = O.pix2sky(wcs, pix, O.WRAP_NONE)
    O.set_threads(1)
    out = np.empty_like(pix)
    for name, arr, fn in (("pix2sky", pix, lambda a, o: O.pix2sky(wcs, a, O.WRAP_UNWIND, out=o)),
                          ("sky2pix", sky_pts, lambda a, o: O.sky2pix(wcs, shape, a, safe=True, out=o))):
        r1, t1 = _cpu_median_rate(lambda: fn(arr[:n1], out[:n1]), n1, 1)
        rN, tN = _cpu_median_rate(lambda: fn(arr, out), nN, cores) if cores > 1 else (r1, t1)
        res[name] = {"value": round(rN / 1e6, 1), "value_1core": round(r1 / 1e6, 1), "scaling_1_to_N": round(rN / r1, 2), "unit": "Mpts/s", "cores": cores,
                     "kind": "port", "runs": 5, "times_s": tN, "times_s_1core": t1,
                     "sample": "oracle %s! on a 2xN batch (car_proj.jl:%s, safe=true) of %d (all-core) / %d (1-core) random points%s" % (
                         name, "92-122 + unwind!, enmap_ops.jl:26-32" if name == "pix2sky" else "165-200", nN, n1,
                         "; the unwrap recurrence is serial in the reference and stays serial here" if name == "pix2sky" else "")}
    return res


if __name__ == "__main__":
    main()
