#!/usr/bin/env python
"""Digests of what the numpy yardsticks under tests/ return, to compare two versions of them bit for bit.

    python tools/yardstick_digests.py --tests-dir tests > new.txt
    python tools/yardstick_digests.py --tests-dir /some/other/checkout/tests > old.txt
    diff old.txt new.txt

The yardstick modules (scatter_ref, nearest_ref, scatter_cubic_ref, pol_ref, normal_ref, destripe_ref) are imported from
--tests-dir; the package and the oracle from this checkout.  Every public function is called on a fixed list of inputs: every
named geometry; nearest_ref.points and the device tests' edge points at n = 2003, each with the three non-finite positions, and
the empty batch; one, three and six planes; with and without an initial map; the whole map, the device tests' row windows with
all points (the raising yardsticks raise) and with points inside the window (they do not), and a window of no rows.  One line
per call: a label and the SHA-256 over dtype, shape and raw bytes of every array returned, or the exception's type and text.
The timestream filters' yardsticks (polyfilter_ref, modefilter_ref) need no geometry: filter in Float64, long double and the
device's order, with and without weights and cuts, on in-range and out-of-range offsets, both solves and both projectors.
CPU only."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2003
WINDOWS = {"cc_360x181": (60, 50), "box_80x40": (7, 20), "box_5x7": (2, 3), "box_2x2": (1, 1), "box_1x1": (0, 1)}          # test_gpu_nearest.WINDOWS
DENSE_MAX = 3200                   # pixels: a dense matrix of P is formed up to here only
NCALLS = [0]


def _feed(h, v):
    if v is None or isinstance(v, (bool, int, float, str)):
        h.update(repr(v).encode())
    elif isinstance(v, (tuple, list)):
        h.update(b"(%d" % len(v))
        for x in v:
            _feed(h, x)
    elif hasattr(v, "indptr"):                      # scipy.sparse CSR
        _feed(h, (v.shape, v.indptr, v.indices, v.data))
    else:
        a = np.ascontiguousarray(v)
        h.update(("%s%r" % (a.dtype.str, a.shape)).encode())
        if a.dtype == np.longdouble and a.dtype.itemsize == 16 and np.finfo(np.longdouble).nmant == 63:
            a = a.reshape(-1).view(np.uint8).reshape(-1, 16)[:, :10]        # x87: the last 6 of the 16 bytes are padding, whatever was there
        h.update(a.tobytes())


def call(label, fn, *args, **kw):
    NCALLS[0] += 1
    try:
        with np.errstate(all="ignore"):
            out = fn(*args, **kw)
        h = hashlib.sha256()
        _feed(h, out)
        print("%-78s %s" % (label, h.hexdigest()))
    except Exception as e:                          # the text is part of what is compared
        print("%-78s %s: %s" % (label, type(e).__name__, e))


def tod_filters():
    """polyfilter_ref and modefilter_ref: 3 x 130 in segments of 1, 2, 8, 64 and 65 samples, 17 x 130 in groups of 1, 2, 15 and 16
    detectors, and offsets that run outside both ways."""
    import modefilter_ref as MF
    import polyfilter_ref as PF
    rng = np.random.default_rng(418)
    nd, nt = 3, 130
    d = rng.normal(size=(nd, nt)) + 50.0 * np.sin(np.arange(nt) / 40.0)
    w = rng.uniform(0.5, 2.0, (nd, nt)) * (rng.uniform(size=(nd, nt)) >= 0.1)
    wn = w.copy()
    wn[1, 5:9] = [np.nan, -1.0, 0.0, np.nan]                       # not live, each its own way
    segs = {"ones": list(range(nt + 1)), "pairs": list(range(0, nt + 1, 2)), "eights": list(range(0, nt + 1, 8)), "wave": [0, 64, 129],
            "outside": [-5, 40, 200, 2 ** 62], "empty": [3, 3, 70, 70, 128]}
    for sname, seg in segs.items():
        call("polyfilter_ref.clamp_segments %s" % sname, PF.clamp_segments, seg, nt)
        for order in (0, 1, 3, 7):
            tag = "polyfilter_ref.filter %s order %d " % (sname, order)
            for wname, wf in (("none", None), ("cuts", w), ("nan", wn)):
                call(tag + wname + " f64", PF.filter, d, seg, order, wfit=wf)
                call(tag + wname + " longdouble", PF.filter, d, seg, order, wfit=wf, dtype=np.longdouble)
                for lanes in sorted({PF.group(nt, len(seg) - 1, order), 2, 64, 256}):
                    call(tag + wname + " lanes %d" % lanes, PF.filter, d, seg, order, wfit=wf, lanes=lanes)
    for L, order in ((12, 3), (65, 7)):
        call("polyfilter_ref.projector %d %d" % (L, order), PF.projector, L, order, rng.uniform(0.25, 4.0, L))
        call("polyfilter_ref.basis %d %d" % (L, order), PF.basis, L, order)
    nd, nt = 17, 130
    d = rng.normal(size=(nd, nt))
    w = rng.uniform(0.5, 2.0, (nd, nt)) * (rng.uniform(size=(nd, nt)) >= 0.1)
    wn = w.copy()
    wn[3:7, 64] = [np.nan, -1.0, 0.0, np.nan]
    grps = {"all": None, "ones": list(range(nd + 1)), "pairs": list(range(0, nd + 1, 2)), "fifteen": [1, 16], "sixteen_one": [0, 16, 17],
            "outside": [-5, 12, 200, 2 ** 62], "empty": [2, 2, 9, 9, 15]}
    for K in (1, 3, 8):
        F = np.concatenate([np.ones((nd, 1)), rng.normal(size=(nd, K - 1))], axis=1)
        d = d + F @ (30.0 * rng.normal(size=(K, nt)))
        for gname, grp in grps.items():
            if grp is not None:
                call("modefilter_ref.clamp_groups %s" % gname, MF.clamp_groups, grp, nd)
            tag = "modefilter_ref.filter %s K %d " % (gname, K)
            for wname, wf in (("none", None), ("cuts", w), ("nan", wn)):
                call(tag + wname + " f64", MF.filter, d, F, grp, wfit=wf)
                call(tag + wname + " longdouble", MF.filter, d, F, grp, wfit=wf, dtype=np.longdouble)
                for phases in (4, 16):
                    call(tag + wname + " phases %d" % phases, MF.filter, d, F, grp, wfit=wf, phases=phases)
        call("modefilter_ref.projector K %d" % K, MF.projector, F, rng.uniform(0.25, 4.0, nd))
    # both solves: full rank, rank lost at the first pivot and at the last
    K, T = 4, 12
    A = rng.normal(size=(K, 6, T))
    G = np.einsum("ikt,jkt->ijt", A, A)
    G[:, :, 3:5] = 0.0
    G[3, :, 5:8], G[:, 3, 5:8] = G[2, :, 5:8], G[:, 2, 5:8]
    G[3, 3, 5:8] = G[2, 2, 5:8]
    b = rng.normal(size=(K, T))
    for dtype in (np.float64, np.longdouble):
        call("modefilter_ref.solve %s" % dtype.__name__, MF.solve, G.astype(dtype), b.astype(dtype), 1e-10, dtype)
        for t in range(T):
            call("polyfilter_ref.solve %s column %d" % (dtype.__name__, t), PF.solve, G[:, :, t].astype(dtype), b[:, t].astype(dtype), 1e-10, dtype)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tests-dir", required=True)
    tests = os.path.abspath(ap.parse_args().tests_dir)
    sys.path[:0] = [tests, ROOT]
    import pixell_jl_amd as pj
    from oracle import oracle as O
    O.lib()
    import destripe_ref as D
    import nearest_ref as NR
    import normal_ref as NM
    import pol_ref as P
    import scatter_cubic_ref as T
    import scatter_ref as R
    import spline_ref as SR
    try:
        from gpu_support import edge_points
    except ImportError:                             # a tree from before gpu_support: test_gpu_normal's copy, non-finite tail included
        from test_gpu_normal import _points
        edge_points = lambda O, wcs, shape, n, seed, nonfinite_tail: _points(O, wcs, shape, n, seed)

    tod_filters()
    geoms = {}
    for mod in (SR, R, T, NR, NM):
        for name, g in mod.geometries(pj).items():
            call("geometry %s.%s" % (mod.__name__, name), lambda g=g: (tuple(g[0]), type(g[1]).__name__, g[1].cdelt, g[1].crpix, g[1].crval))
            geoms.setdefault(name, g)

    for name in sorted(geoms):
        shape, wcs = geoms[name]
        shape = (int(shape[0]), int(shape[1]))
        nx, ny = shape
        rng = np.random.default_rng(len(name))
        row0, nrows = WINDOWS.get(name, (ny // 3, max(1, ny // 2)))
        batches = {"points": NR.points(O, wcs, shape, N, 5), "edge": edge_points(O, wcs, shape, N, 6, True), "empty": np.zeros((0, 2))}
        if nrows >= 6:
            pix = np.stack([rng.uniform(1, nx, N), rng.uniform(row0 + 3, row0 + nrows - 2, N)], axis=1)
            batches["inside"] = O.pix2sky(wcs, pix, O.WRAP_NONE)
        for bname, sky in batches.items():
            n = len(sky)
            resp, w, d = rng.normal(size=(n, 2)), 10.0 ** rng.uniform(-1, 1, n), rng.normal(size=n)
            vals = {1: rng.normal(size=n), 3: rng.normal(size=(3, n)), 6: rng.normal(size=(6, n))}
            vals[3][:, ::7] = 0.0                               # zero terms, for nonzero_terms
            dz = np.where(np.arange(n) % 5 == 0, 0.0, d)
            for wname, win in (("full", {}), ("window", {"row0": row0, "nrows": nrows}), ("no rows", {"row0": ny // 2, "nrows": 0})):
                if bname == "inside" and wname != "window":
                    continue
                nr = win.get("nrows", ny)
                tag = "%s %s %s " % (name, bname, wname)
                m3, m6 = rng.normal(size=(3, nr, nx)), rng.normal(size=(6, nr, nx))
                mask = (rng.uniform(size=(nr, nx)) > 0.2).astype(np.float64)
                call(tag + "scatter_ref.taps", R.taps, O, wcs, shape, sky, **win)
                call(tag + "nearest_ref.cells", NR.cells, O, wcs, shape, sky, **win)
                call(tag + "nearest_ref.taps", NR.taps, O, wcs, shape, sky, **win)
                call(tag + "scatter_cubic_ref.taps", T.taps, O, wcs, shape, sky, **win)
                call(tag + "nearest_ref.sample", NR.sample, O, wcs, shape, m3, sky, **win)
                call(tag + "nearest_ref.sample_pol", NR.sample_pol, O, wcs, shape, m3, sky, resp, **win)
                for order, pre in ((1, False), (3, True)):
                    call(tag + "pol_ref.sample_planes order %d" % order, P.sample_planes, O, wcs, shape, m3, sky, order, pre, **win)
                    call(tag + "pol_ref.sample order %d" % order, P.sample, O, wcs, shape, m3, sky, resp, order, pre, **win)
                for nc, v in vals.items():
                    for oname, out in (("zeros", None), ("out", rng.normal(size=(nc, nr, nx)))):
                        for mod in (R, NR, T):
                            call(tag + "%s.scatter nc=%d %s" % (mod.__name__, nc, oname), mod.scatter, O, wcs, shape, sky, v, out=out, **win)
                    call(tag + "nearest_ref.nonzero_terms nc=%d" % nc, NR.nonzero_terms, O, wcs, shape, sky, v, **win)
                    if not win:
                        call(tag + "scatter_cubic_ref.nonzero_terms nc=%d" % nc, T.nonzero_terms, O, wcs, shape, sky, v)
                for mode, mp in ((0, m3), (1, m6)):
                    for oname, out in (("zeros", None), ("out", mp)):
                        call(tag + "nearest_ref.scatter_pol mode %d %s" % (mode, oname), NR.scatter_pol, O, wcs, shape, sky, dz, resp, mode, out=out, **win)
                        for order in (1, 3):
                            call(tag + "pol_ref.scatter order %d mode %d %s" % (order, mode, oname), P.scatter, O, wcs, shape, sky, dz, resp, order, mode,
                                 out=out, **win)
                    call(tag + "nearest_ref.nonzero_terms_pol mode %d" % mode, NR.nonzero_terms_pol, O, wcs, shape, sky, dz, resp, mode, **win)
                    call(tag + "pol_ref.nonzero_terms order 1 mode %d" % mode, P.nonzero_terms, O, wcs, shape, sky, dz, resp, 1, mode, **win)
                    if not win:
                        call(tag + "pol_ref.nonzero_terms order 3 mode %d" % mode, P.nonzero_terms, O, wcs, shape, sky, dz, resp, 3, mode)
                        for order in (1, 3):
                            call(tag + "pol_ref.scatter_full order %d mode %d" % (order, mode), P.scatter_full, O, wcs, shape, sky, d, resp, order, mode)
                for oname, out in (("zeros", None), ("out", m3)):
                    call(tag + "nearest_ref.bin " + oname, NR.bin, O, wcs, shape, sky, resp, d, w, rhs=out, weights=None if out is None else m6, **win)
                    call(tag + "normal_ref.normal " + oname, NM.normal, O, wcs, shape, m3, sky, resp, w, out=out, **win)
                # destripe_ref: the batch as nd = 1 detector (2 where n is even), baselines of 37 samples
                nd = 2 if n and n % 2 == 0 else 1
                nb = D.n_base(max(n // nd, 1), 37)
                a = rng.normal(size=nd * nb)
                for mname, mk in (("", None), (" mask", mask)):
                    for oname, out3, outb in (("zeros", None, None), ("out", m3, rng.normal(size=nd * nb))):
                        call(tag + "destripe_ref.bin%s %s" % (mname, oname), D.bin, O, wcs, shape, sky, resp, w, nd, 0, 37, nb, d=d, a=a, mask=mk,
                             out=out3, **win)
                        call(tag + "destripe_ref.project%s %s" % (mname, oname), D.project, O, wcs, shape, sky, resp, w, nd, 0, 37, nb, d=d, m=m3,
                             mask=mk, out=outb, **win)
                    call(tag + "destripe_ref.project%s a only" % mname, D.project, O, wcs, shape, sky, resp, w, nd, 0, 37, nb, a=a, mask=mk, **win)
                if win:
                    continue
                call(tag + "nearest_ref.classes", NR.classes, O, wcs, shape, sky)
                call(tag + "normal_ref.sparse_p", NM.sparse_p, O, wcs, shape, sky, resp)
                call(tag + "nearest_ref.blocks_bound", NR.blocks_bound, O, wcs, shape, m3, sky, resp, w)
                if nx * ny <= DENSE_MAX:
                    call(tag + "nearest_ref.dense", NR.dense, O, wcs, shape, sky)
                    call(tag + "nearest_ref.dense resp", NR.dense, O, wcs, shape, sky, resp)
                    for order in (1, 3):
                        call(tag + "pol_ref.dense order %d" % order, P.dense, O, wcs, shape, sky, resp, order)

                def gaps():                                 # the adjoint gaps on finite positions, as their tests call them
                    keep = NR.cells(O, wcs, shape, sky)[1]
                    s, dk, rk = sky[keep], d[keep], resp[keep]
                    m1 = m3[:1]
                    ref, k, S = R.scatter(O, wcs, shape, s, dk)
                    out = [R.adjoint_gap(m1, P.sample_planes(O, wcs, shape, m1, s), dk, ref, k, S)]
                    ref, k, S = NR.scatter(O, wcs, shape, s, dk)
                    pm = NR.sample(O, wcs, shape, m1, s)
                    out.append(NR.adjoint_gap(m1, pm, dk, ref, k, S))
                    ref, k, S = NR.scatter_pol(O, wcs, shape, s, dk, rk)
                    p3 = NR.sample(O, wcs, shape, m3, s)
                    out.append(NR.adjoint_gap_pol(m3, NR.sample_pol(O, wcs, shape, m3, s, rk), dk, ref, k, S, p3, rk))
                    return out
                call(tag + "adjoint_gap, adjoint_gap (nearest), adjoint_gap_pol", gaps)
    print("calls: %d" % NCALLS[0])


if __name__ == "__main__":
    main()
