#!/usr/bin/env python3
"""One run of the tile-kernel instantiations whose assembly differs from the parent's: median launch time of each, as one
JSON line.  The library is whatever PXL_LIB_PATH names (the tree's own by default); one process per run."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import pixell_jl_amd as pj  # noqa: E402

dev = torch.device("cuda:0")
pj.load_library()


def wcs(nx, dy, crpix_y, ra0=0.3):
    return pj.CarClenshawCurtis((-360.0 / nx, dy), (nx / 2 + 0.25, crpix_y), (ra0, 0.0))


def time_plan(shape_in, wcs_in, shape_out, wcs_out, dtype, variant, offset8, rounds=15):
    nx, ny, nc = shape_in
    nxo, nyo = shape_out
    n = nc * ny * nx
    pad = 8 // torch.empty((), dtype=dtype).element_size()
    owner = torch.randn(n + 2 * pad, dtype=dtype, device=dev)
    src = (owner[pad:pad + n] if offset8 else owner[:n]).view(nc, ny, nx)
    assert src.data_ptr() % 16 == (8 if offset8 else 0)
    plan = pj.ReprojectPlan(shape_in, wcs_in, shape_out, wcs_out, device=dev)
    plan.set_variant(variant)
    dst = torch.empty(plan.dst_tensor_shape(), dtype=dtype, device=dev)
    plan.build_tables()
    for _ in range(3):
        plan.execute_rows(src, dst, 0, nyo)
    torch.cuda.synchronize()
    t = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.execute_rows(src, dst, 0, nyo)
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1))
    plan.close()
    return sorted(t)[len(t) // 2]


out = {"lib": os.environ.get("PXL_LIB_PATH", "tree")}
# k_reproject_dma<T, PAIRS, 1>: a 5x RA refinement (sx = 0.2), slots of at most one 1-KiB access at every lane width
nx_in, ny_in, nxo, nyo = 2160, 1200, 10800, 1200
gi, go = ((nx_in, ny_in, 1), wcs(nx_in, 0.1, 600.0)), ((nxo, nyo), wcs(nxo, 0.1, 600.3))
for dtype, tag in ((torch.float64, "d"), (torch.float32, "f")):
    for pairs in (1, 2, 4):
        os.environ["PXL_REPROJECT_PAIRS"] = str(pairs)
        out["dma<%s,%d,1>" % (tag, pairs)] = time_plan(gi[0], gi[1], go[0], go[1], dtype, 0, False)
# k_reproject_staged<PAIRS, VEC>: variant 2 at equal resolution; VEC = false from a source 8 bytes off a 16-byte boundary
nx_in, ny_in = 8192, 2049
gi, go = ((nx_in, ny_in, 1), wcs(nx_in, 180.0 / 2048, 1025.0)), ((nx_in, ny_in), wcs(nx_in, 180.0 / 2048, 1025.5, ra0=0.32))
for pairs in (1, 2):
    os.environ["PXL_REPROJECT_PAIRS"] = str(pairs)
    for vec in (True, False):
        out["staged<%d,%s>" % (pairs, "true" if vec else "false")] = time_plan(gi[0], gi[1], go[0], go[1], torch.float64, 2, not vec)
print(json.dumps(out))
