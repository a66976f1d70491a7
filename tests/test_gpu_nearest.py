"""Nearest-pixel (order 0) pointing on the device: pj.sample_nearest, pj.scatter_nearest, their polarised forms,
pj.bin_pol_nearest and the five C entries behind them, against the numpy yardstick tests/nearest_ref.py.

The forwards copy a pixel (and combine three), so they are compared as BIT PATTERNS.  The transposes add by hardware atomics in an
unspecified order, so they are held to k * 2^-52 * S per pixel (scatter_ref's derivation) against the yardstick's (ref, k, S), to
the yardstick's bits wherever at most one non-zero term lands, and to the initial map's bits wherever nothing lands.  The fused
pass is held the same way against the yardstick AND against the device's own composition.  Two device calls are never asserted
bit-equal beyond that.  Each check prints its worst error / bound."""
import ctypes as C

import numpy as np
import pytest

import nearest_ref as N
import scatter_ref as R

torch = pytest.importorskip("torch")
from gpu_support import bits, dev, held_inf, out0_idle, same_bits, to_dev
pytestmark = pytest.mark.gpu

CHUNK = 1024                     # the points one block takes per trip, every kernel: blockDim.x (256) times PXL_ZUNR = 4
NPTS = 20011                     # 20 blocks, the last partial
WINDOWS = {"cc_360x181": (60, 50), "box_80x40": (7, 20), "box_5x7": (2, 3), "box_2x2": (1, 1), "box_1x1": (0, 1)}


def _transpose_check(got, out0, triple, nz, what, others=()):
    """got against the yardstick's triple (and any other device results of the same terms): the bound everywhere, the yardstick's
    bits where at most one non-zero term lands, the initial map's bits where nothing lands.  Returns (single, idle) counts."""
    ref, k, S = triple
    got = np.asarray(got).reshape(ref.shape)
    held_inf(got, ref, k, S, what + " against the yardstick")
    for o in others:
        held_inf(got, np.asarray(o).reshape(ref.shape), k, S, what + " against the composition")
    single = nz <= 1
    for other in (ref,) + tuple(np.asarray(o).reshape(ref.shape) for o in others):
        same_bits(got[single], other[single], what + ": a pixel with at most one non-zero term")
    idle = k == 1
    assert np.array_equal(bits(got[idle]), bits(out0.reshape(ref.shape)[idle])), what + ": a pixel that receives nothing changed"
    return int(single.sum()), int(idle.sum())


def _case(pj, O, geom, n, seed, sparse=False):
    """Points, responses, values and weights.  sparse: only the first 48 points and the non-finite ones, so that pixels are left
    alone on the small maps too."""
    shape, wcs = N.geometries(pj)[geom]
    sky = N.points(O, wcs, shape, n, seed)
    if sparse:
        sky = np.concatenate([sky[:48], sky[-3:]])
    rng = np.random.default_rng(seed + 7)
    n = len(sky)
    resp, vals, w = rng.normal(size=(n, 2)), rng.normal(size=(3, n)), 10.0 ** rng.uniform(-1, 1, n)
    idx = N.taps(O, wcs, shape, sky)[0]
    if n >= 3:
        vals[:, -3:] = np.nan                                  # positions that are not finite: the value must go nowhere
        w[-3:] = np.nan
    return shape, wcs, sky, resp, vals, w, idx


# ---- 1. forward bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", N.GEOMS)
def test_forward_bits(pj, O, dev, geom):
    """sample_nearest (1, 2 and 3 planes) and sample_pol_nearest are the yardstick's bit patterns on a map that holds NaN, +-Inf,
    -0.0, huge and subnormal pixels; NaN exactly where the position is not finite, +0.0 off the map; the same on a row window."""
    shape, wcs, sky, resp, _vals, _w, idx = _case(pj, O, geom, NPTS, 101)
    fin = np.isfinite(sky).all(axis=1)
    dsky, dresp = to_dev(sky, dev), to_dev(resp, dev)
    m = N.special_map(shape, 3, 102)
    for nc in (3, 2, 1):
        data = m[:nc] if nc > 1 else m[0]
        got = pj.sample_nearest(pj.Enmap(to_dev(data, dev), wcs), dsky).cpu().numpy()
        assert got.shape == (nc, NPTS)
        assert np.array_equal(bits(got), bits(N.sample(O, wcs, shape, data, sky))), "%s, %d planes: not the pixel's bits" % (geom, nc)
    clean = np.where(np.isfinite(m) & (np.abs(m) < 1e300), m, 1.0)          # nothing that overflows in the combination
    clean[clean == 0] = 2.0
    got = pj.sample_nearest(pj.Enmap(to_dev(clean, dev), wcs), dsky).cpu().numpy()
    assert np.array_equal(np.isnan(got[0]), ~fin) and (~fin).sum() == 3
    off = fin & (idx < 0)
    assert off.any() and not bits(got[:, off]).any(), "a point off the map is not +0.0"
    assert (got[:, fin & (idx >= 0)] != 0).all()
    with np.errstate(invalid="ignore", over="ignore"):
        want = N.sample_pol(O, wcs, shape, m, sky, resp)
    gp = pj.sample_pol_nearest(pj.Enmap(to_dev(m, dev), wcs), dsky, dresp).cpu().numpy()
    same_bits(gp, want, geom + ": sample_pol_nearest")
    gc = pj.sample_pol_nearest(pj.Enmap(to_dev(clean, dev), wcs), dsky, dresp).cpu().numpy()
    same_bits(gc, N.sample_pol(O, wcs, shape, clean, sky, resp), geom + ": sample_pol_nearest on a finite map")
    assert np.array_equal(np.isnan(gc), ~fin)
    row0, nrows = WINDOWS[geom]
    strip = np.ascontiguousarray(m[:, row0:row0 + nrows])
    got = pj.sample_nearest(pj.Enmap(to_dev(strip, dev), wcs), dsky, src_rows=(row0, nrows), full_shape=shape).cpu().numpy()
    assert np.array_equal(bits(got), bits(N.sample(O, wcs, shape, strip, sky, row0, nrows)))
    gp = pj.sample_pol_nearest(pj.Enmap(to_dev(strip, dev), wcs), dsky, dresp, src_rows=(row0, nrows), full_shape=shape).cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        same_bits(gp, N.sample_pol(O, wcs, shape, strip, sky, resp, row0, nrows), geom + ": sample_pol_nearest on a window")
    print("%s: %d points, %d off the map, %d on ties" % (geom, NPTS, int(off.sum()), int((N.classes(O, wcs, shape, sky)[0] == 0).sum())))


# ---- 2. pixel edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", N.GEOMS)
def test_pixel_edges(pj, O, dev, geom):
    """Every x = i + 0.5, y = j + 0.5 for i in [-1, nx + 1], j in [-1, ny + 1], as it is and moved by -+2^-30 pixel: the sampler
    returns the pixel the yardstick names (the map holds each pixel's own number) and the hit counts are the yardstick's exactly
    -- ties go up, x = nx + 0.5 is column 1 of the periodic map and off a box, y = 0.5 is row 1, y = ny + 0.5 is off the map."""
    shape, wcs = N.geometries(pj)[geom]
    nx, ny = shape
    sky = np.concatenate([N.edge_points(O, wcs, shape, s) for s in (0.0, -N.NUDGE, N.NUDGE)])
    cx, cy = N.classes(O, wcs, shape, sky)
    need = 16 if geom not in ("box_1x1", "box_2x2") else 9
    for cls in (0, -1, 1):
        assert (cx == cls).sum() >= need and (cy == cls).sum() >= need, "%s: class %d is short of points" % (geom, cls)
    assert len(sky) == 3 * (nx + 3) * (ny + 3) and ((cx == 0) == (cy == 0)).all()
    numbered = np.arange(1.0, nx * ny + 1).reshape(ny, nx)
    got = pj.sample_nearest(pj.Enmap(to_dev(numbered, dev), wcs), to_dev(sky, dev)).cpu().numpy()[0]
    idx = N.taps(O, wcs, shape, sky)[0]
    assert np.array_equal(got, np.where(idx >= 0, idx + 1.0, 0.0)), geom + ": a point lands on another pixel than the yardstick's"
    hits = pj.scatter_nearest(to_dev(np.ones(len(sky)), dev), to_dev(sky, dev), shape, wcs).data.cpu().numpy()
    want = np.bincount(idx[idx >= 0], minlength=nx * ny).reshape(ny, nx)
    assert np.array_equal(hits, want.astype(np.float64)), geom + ": hit counts differ"
    tie = (cx == 0)
    print("%s: %d edge points, %d ties, %d on the map" % (geom, len(sky), int(tie.sum()), int((idx >= 0).sum())))
    # the tie's pixel is the +2^-30 neighbour's, not the -2^-30 one's (where the two differ at all)
    third = len(sky) // 3
    assert np.array_equal(idx[:third], idx[2 * third:]) and (idx[:third] != idx[third:2 * third]).any()


# ---- 3. transposes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("geom", N.GEOMS)
def test_transposes(pj, O, dev, geom, sparse):
    """scatter_nearest (1, 2, 3 planes), scatter_pol_nearest and scatter_pol_weights_nearest accumulate into a non-trivial map:
    the bound, the single-term bits, the untouched pixels' bits (-0.0 and NaN among them).  One value is NaN: it reaches exactly
    its one pixel per plane.  The points whose position is not finite carry NaN values, which must go nowhere."""
    shape, wcs, sky, resp, vals, w, idx = _case(pj, O, geom, NPTS, 111, sparse)
    nx, ny = shape
    on = np.flatnonzero(idx >= 0)
    vals[:, on[len(on) // 2]] = np.nan
    nan_pix = idx[on[len(on) // 2]]
    idle = np.bincount(idx[idx >= 0], minlength=nx * ny).reshape(ny, nx) == 0
    if geom == "cc_360x181" or (sparse and geom == "box_80x40"):
        assert idle.sum() >= 64
    dsky, dresp = to_dev(sky, dev), to_dev(resp, dev)
    for nc in (1, 2, 3):
        out0 = out0_idle(nc, ny, nx, idle, 112 + nc)
        v = vals[:nc] if nc > 1 else vals[0]
        dst = to_dev(out0 if nc > 1 else out0[0], dev)
        res = pj.scatter_nearest(to_dev(v, dev), dsky, shape, wcs, out=dst)
        assert isinstance(res, pj.Enmap) and res.data.data_ptr() == dst.data_ptr()
        got = dst.cpu().numpy()
        s, i = _transpose_check(got, out0, N.scatter(O, wcs, shape, sky, v, out=out0), N.nonzero_terms(O, wcs, shape, sky, v),
                                "%s, %d planes" % (geom, nc))
        nan_new = np.isnan(got.reshape(nc, -1)) & ~np.isnan(out0.reshape(nc, -1))
        assert np.array_equal(np.flatnonzero(nan_new[0]), [nan_pix]) and (nan_new == nan_new[0]).all(), "the NaN value is not in exactly its pixel"
    fresh = pj.scatter_nearest(to_dev(vals[0], dev), dsky, shape, wcs)
    assert tuple(fresh.data.shape) == (ny, nx)
    held_inf(fresh.data.cpu().numpy()[None], *N.scatter(O, wcs, shape, sky, vals[0]), geom + ", fresh map")
    for mode, fn, v in ((0, pj.scatter_pol_nearest, vals[0]), (1, pj.scatter_pol_weights_nearest, w)):
        planes = 6 if mode else 3
        out0 = out0_idle(planes, ny, nx, idle, 120 + mode)
        dst = to_dev(out0, dev)
        fn(to_dev(v, dev), dsky, dresp, shape, wcs, out=dst)
        s, i = _transpose_check(dst.cpu().numpy(), out0, N.scatter_pol(O, wcs, shape, sky, v, resp, mode, out=out0),
                                N.nonzero_terms_pol(O, wcs, shape, sky, v, resp, mode), "%s, polarised mode %d" % (geom, mode))
    print("%s: %d pixels with at most one non-zero term, %d untouched" % (geom, s, i))


@pytest.mark.parametrize("geom", N.GEOMS)
def test_transposes_on_a_row_window(pj, O, dev, geom):
    shape, wcs, sky, resp, vals, w, _idx = _case(pj, O, geom, NPTS, 131)
    nx, ny = shape
    row0, nrows = WINDOWS[geom]
    widx = N.taps(O, wcs, shape, sky, row0, nrows)[0]
    idle = np.bincount(widx[widx >= 0], minlength=nx * nrows).reshape(nrows, nx) == 0
    dsky, dresp = to_dev(sky, dev), to_dev(resp, dev)
    kw = dict(src_rows=(row0, nrows), full_shape=shape)
    out0 = out0_idle(3, nrows, nx, idle, 132)
    dst = to_dev(out0, dev)
    pj.scatter_nearest(to_dev(vals, dev), dsky, shape, wcs, out=dst, **kw)
    _transpose_check(dst.cpu().numpy(), out0, N.scatter(O, wcs, shape, sky, vals, out=out0, row0=row0, nrows=nrows),
                     N.nonzero_terms(O, wcs, shape, sky, vals, row0, nrows), geom + ", window")
    for mode, fn, v in ((0, pj.scatter_pol_nearest, vals[0]), (1, pj.scatter_pol_weights_nearest, w)):
        out0 = out0_idle(6 if mode else 3, nrows, nx, idle, 133 + mode)
        dst = to_dev(out0, dev)
        fn(to_dev(v, dev), dsky, dresp, shape, wcs, out=dst, **kw)
        _transpose_check(dst.cpu().numpy(), out0, N.scatter_pol(O, wcs, shape, sky, v, resp, mode, out=out0, row0=row0, nrows=nrows),
                         N.nonzero_terms_pol(O, wcs, shape, sky, v, resp, mode, row0, nrows), "%s, window, mode %d" % (geom, mode))
    assert (N.taps(O, wcs, shape, sky)[0] >= 0).sum() >= (widx >= 0).sum() > 0


# ---- 4. the fused contract ----------------------------------------------------------------------------------------------------------
def _fused_check(pj, O, dev, shape, wcs, sky, resp, d, w, what, seed, batches=1):
    """bin_pol_nearest into non-trivial maps against the yardstick's two triples and the device's own composition; the II plane
    against scatter_nearest(w).  With batches = 2 the points go in two calls into the same maps."""
    nx, ny = shape
    idx = N.taps(O, wcs, shape, sky)[0]
    idle = np.bincount(idx[idx >= 0], minlength=nx * ny).reshape(ny, nx) == 0
    rhs0, wts0 = out0_idle(3, ny, nx, idle, seed), out0_idle(6, ny, nx, idle, seed + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        tr, tw = N.bin(O, wcs, shape, sky, resp, d, w, rhs=rhs0, weights=wts0)
        wd = np.asarray(w) * np.asarray(d)
        nzr, nzw = N.nonzero_terms_pol(O, wcs, shape, sky, wd, resp, 0), N.nonzero_terms_pol(O, wcs, shape, sky, w, resp, 1)
    dsky, dresp, dd, dw = to_dev(sky, dev).reshape(-1, 2), to_dev(resp, dev).reshape(-1, 2), to_dev(d, dev), to_dev(w, dev)
    comp_r = pj.scatter_pol_nearest(dw * dd, dsky, dresp, shape, wcs, out=to_dev(rhs0, dev)).data.cpu().numpy()
    comp_w = pj.scatter_pol_weights_nearest(dw, dsky, dresp, shape, wcs, out=to_dev(wts0, dev)).data.cpu().numpy()
    ii = pj.scatter_nearest(dw, dsky, shape, wcs, out=to_dev(wts0[0], dev)).data.cpu().numpy()
    rhs, wts = to_dev(rhs0, dev), to_dev(wts0, dev)
    n = len(d)
    cuts = np.linspace(0, n, batches + 1).astype(int)
    for a, b in zip(cuts[:-1], cuts[1:]):
        r1, w1 = pj.bin_pol_nearest(dd[a:b], dw[a:b], dsky[a:b], dresp[a:b], shape, wcs, rhs=rhs, weights=wts)
        assert isinstance(r1, pj.Enmap) and r1.data.data_ptr() == rhs.data_ptr() and w1.data.data_ptr() == wts.data_ptr()
    torch.cuda.synchronize()
    gr, gw = rhs.cpu().numpy(), wts.cpu().numpy()
    sr = _transpose_check(gr, rhs0, tr, nzr, what + ", rhs", others=(comp_r,))
    sw = _transpose_check(gw, wts0, tw, nzw, what + ", weights", others=(comp_w,))
    held_inf(gw[:1], ii[None], tw[1][:1], tw[2][:1], what + ", II plane against scatter_nearest(w)")
    return gr, gw, tr, tw, sr, sw


@pytest.mark.parametrize("geom", N.GEOMS)
def test_fused_contract(pj, O, dev, geom):
    shape, wcs, sky, resp, vals, w, idx = _case(pj, O, geom, NPTS, 141)
    d = vals[1]
    w[5] = 0.0; resp[6] = [0.0, 1.5]                                  # zero terms still add, and change nothing
    w[-3:] = 1.0; d[-3:] = 1.0                                        # finite values on positions that are not: they add nothing
    gr, gw, tr, tw, sr, sw = _fused_check(pj, O, dev, shape, wcs, sky, resp, d, w, geom, 142)
    print("%s: rhs %d single-term and %d untouched pixels, weights %d and %d" % ((geom,) + sr + sw))
    assert np.isfinite(gr[~np.isnan(tr[0])]).all()
    _fused_check(pj, O, dev, shape, wcs, sky, resp, d, w, geom + ", two batches", 144, batches=2)
    # rhs = weights = None are maps of zeros
    r, wt = pj.bin_pol_nearest(to_dev(d, dev), to_dev(w, dev), to_dev(sky, dev), to_dev(resp, dev), shape, wcs)
    assert tuple(r.data.shape) == (3, shape[1], shape[0]) and tuple(wt.data.shape) == (6, shape[1], shape[0])
    t0r, t0w = N.bin(O, wcs, shape, sky, resp, d, w)
    held_inf(r.data.cpu().numpy(), *t0r, geom + ", fresh rhs")
    held_inf(wt.data.cpu().numpy(), *t0w, geom + ", fresh weights")


def test_fused_special_values(pj, O, dev):
    """A NaN sample, an infinite sample and a NaN weight: each reaches exactly its one pixel -- the NaN weight in all nine planes,
    the samples in the three of rhs -- as in the composition."""
    shape, wcs, sky, resp, vals, w, idx = _case(pj, O, "box_80x40", NPTS, 151)
    d = vals[2]
    w[-3:] = 1.0; d[-3:] = 1.0
    on = np.flatnonzero(idx >= 0)
    a, b, c = on[100], on[2000], on[7000]
    assert len({idx[a], idx[b], idx[c]}) == 3
    d[a], d[b], w[c] = np.nan, np.inf, np.nan
    gr, gw, tr, tw, _sr, _sw = _fused_check(pj, O, dev, shape, wcs, sky, resp, d, w, "special values", 152)
    bad_r = ~np.isfinite(gr.reshape(3, -1)) & (tr[1].reshape(3, -1) > 1)          # among the pixels that received something
    assert set(np.flatnonzero(bad_r.any(axis=0))) == {idx[a], idx[b], idx[c]}
    assert set(np.flatnonzero(np.isnan(gw.reshape(6, -1)).all(axis=0))) >= {idx[c]} and np.isfinite(gw.reshape(6, -1)[:, [idx[a], idx[b]]]).all()


# ---- 5. batch guards and contention -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_batch_sizes(pj, O, dev, n):
    """Every kernel at the sizes round its chunk (256 threads times 4 points): the lanes past the batch read nothing and add
    nothing."""
    shape, wcs = N.geometries(pj)["cc_360x181"]
    nx, ny = shape
    sky = R.sphere_points(n, n + 1).reshape(-1, 2)
    rng = np.random.default_rng(160 + n)
    resp, vals, w = rng.normal(size=(n, 2)), rng.normal(size=(2, n)), 10.0 ** rng.uniform(-1, 1, n)
    m = rng.normal(size=(3, ny, nx))
    dsky, dresp = to_dev(sky, dev).reshape(-1, 2), to_dev(resp, dev).reshape(-1, 2)
    em = pj.Enmap(to_dev(m, dev), wcs)
    got = pj.sample_nearest(em, dsky).cpu().numpy()
    assert got.shape == (3, n) and np.array_equal(bits(got), bits(N.sample(O, wcs, shape, m, sky)))
    got = pj.sample_pol_nearest(em, dsky, dresp).cpu().numpy()
    assert got.shape == (n,) and np.array_equal(bits(got), bits(N.sample_pol(O, wcs, shape, m, sky, resp)))
    idle = np.ones((ny, nx), bool)
    out0 = out0_idle(2, ny, nx, idle & False, 161)
    dst = to_dev(out0, dev)
    pj.scatter_nearest(to_dev(vals, dev).reshape(2, n), dsky, shape, wcs, out=dst)
    tri = N.scatter(O, wcs, shape, sky, vals.reshape(2, n), out=out0)
    _transpose_check(dst.cpu().numpy(), out0, tri, N.nonzero_terms(O, wcs, shape, sky, vals.reshape(2, n)), "n = %d, scalar" % n)
    assert int((tri[1] > 1).sum()) <= 2 * n and (n == 0 or int((tri[1] > 1).sum()) >= 2)
    for mode, fn, v in ((0, pj.scatter_pol_nearest, vals[0]), (1, pj.scatter_pol_weights_nearest, w)):
        out0 = out0_idle(6 if mode else 3, ny, nx, idle & False, 162 + mode)
        dst = to_dev(out0, dev)
        fn(to_dev(v, dev).reshape(n), dsky, dresp, shape, wcs, out=dst)
        _transpose_check(dst.cpu().numpy(), out0, N.scatter_pol(O, wcs, shape, sky, v, resp, mode, out=out0),
                         N.nonzero_terms_pol(O, wcs, shape, sky, v, resp, mode), "n = %d, mode %d" % (n, mode))
    gr, gw, tr, tw, _sr, _sw = _fused_check(pj, O, dev, shape, wcs, sky, resp, vals[1].reshape(n), w, "n = %d, fused" % n, 165)
    assert int((tr[1] > 1).sum()) <= 3 * n and int((tw[1] > 1).sum()) <= 6 * n


@pytest.mark.parametrize("pattern", ["one pixel", "a row in scan order"])
def test_contention(pj, O, dev, pattern):
    """10^5 points in one pixel, and 10^5 points in scan order along one row: every transpose within the bound, with k up to
    10^5 + 1 in a pixel."""
    shape, wcs = N.geometries(pj)["cc_360x181"]
    nx, ny = shape
    n = 10 ** 5
    rng = np.random.default_rng(171)
    if pattern == "one pixel":
        pix = np.stack([rng.uniform(99.501, 100.499, n), rng.uniform(49.501, 50.499, n)], axis=1)
    else:
        pix = np.stack([np.linspace(0.6, nx + 0.4, n), np.full(n, 50.25)], axis=1)
    sky = O.pix2sky(wcs, pix, O.WRAP_NONE)
    resp, d, w = rng.normal(size=(n, 2)), rng.normal(size=n), 10.0 ** rng.uniform(-1, 1, n)
    idx = N.taps(O, wcs, shape, sky)[0]
    assert (idx >= 0).all() and len(np.unique(idx)) == (1 if pattern == "one pixel" else nx)
    idle = np.zeros((ny, nx), bool)
    out0 = out0_idle(1, ny, nx, idle, 172)
    dst = to_dev(out0[0], dev)
    pj.scatter_nearest(to_dev(d, dev), to_dev(sky, dev), shape, wcs, out=dst)
    tri = N.scatter(O, wcs, shape, sky, d, out=out0)
    _transpose_check(dst.cpu().numpy(), out0, tri, N.nonzero_terms(O, wcs, shape, sky, d), pattern + ", scalar")
    gr, gw, tr, tw, _sr, _sw = _fused_check(pj, O, dev, shape, wcs, sky, resp, d, w, pattern + ", fused", 173)
    assert int(tw[1].max()) == (n + 1 if pattern == "one pixel" else int(np.bincount(idx).max()) + 1)
    assert int((tw[1] > 1).sum()) == 6 * len(np.unique(idx))


# ---- 6. adjoint ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", N.GEOMS)
def test_adjoint(pj, O, dev, geom):
    """<P m, d> = <m, P^T d> on the device's own outputs, scalar and polarised, within the bound from the yardstick's (k, S)."""
    shape, wcs, sky, resp, vals, _w, _idx = _case(pj, O, geom, NPTS, 181)
    keep = np.isfinite(sky).all(axis=1)
    sky, resp, d = sky[keep], resp[keep], vals[0][keep]
    m = np.random.default_rng(182).normal(size=(3, shape[1], shape[0]))
    dsky, dresp, em = to_dev(sky, dev), to_dev(resp, dev), pj.Enmap(to_dev(m, dev), wcs)
    pm = pj.sample_nearest(em, dsky).cpu().numpy()
    d3 = np.stack([d, d, d])
    ptd = pj.scatter_nearest(to_dev(d3, dev), dsky, shape, wcs).data.cpu().numpy()
    _ref, k, S = N.scatter(O, wcs, shape, sky, d3)
    gap, b = N.adjoint_gap(m, pm, d, ptd, k, S)
    print("%s: scalar adjoint gap %.3g, bound %.3g" % (geom, gap, b))
    assert gap <= b
    pmp = pj.sample_pol_nearest(em, dsky, dresp).cpu().numpy()
    ptdp = pj.scatter_pol_nearest(to_dev(d, dev), dsky, dresp, shape, wcs).data.cpu().numpy()
    _ref, kp, Sp = N.scatter_pol(O, wcs, shape, sky, d, resp)
    gap, b = N.adjoint_gap_pol(m, pmp, d, ptdp, kp, Sp, pm, resp)
    print("%s: polarised adjoint gap %.3g, bound %.3g" % (geom, gap, b))
    assert gap <= b


# ---- 7. the raw ABI -----------------------------------------------------------------------------------------------------------------
def test_einval_leaves_every_buffer_untouched(pj, dev):
    lib = pj.load_library()
    L = pj._lib
    shape, wcs = N.geometries(pj)["cc_360x181"]
    wc = wcs.to_struct()
    n, npl = 2000, 181 * 360
    rhs = torch.full((4, 181, 360), -3.5, dtype=torch.float64, device=dev)       # a plane to spare for the overlap cases
    wts = torch.full((7, 181, 360), 2.5, dtype=torch.float64, device=dev)
    src = torch.full((3, 181, 360), 1.25, dtype=torch.float64, device=dev)
    sky = torch.full((n, 2), 0.25, dtype=torch.float64, device=dev)              # on the map: a call that ran would add
    resp = torch.full((n, 2), 0.75, dtype=torch.float64, device=dev)
    d = torch.full((n,), 2.0, dtype=torch.float64, device=dev)
    w = torch.full((n,), 1.5, dtype=torch.float64, device=dev)
    out = torch.full((3, n), 9.0, dtype=torch.float64, device=dev)
    P_ = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    W = C.byref(wc)
    shp = L.shape_arr((360, 181, 3))
    bad_wcs = type(wc)()
    fn = lib.pxl_bin_car_pol_nearest_f64
    good = (W, shp, P_(rhs), P_(wts), n, P_(sky), P_(resp), P_(d), P_(w))

    def swap(pos, val, base=good):
        a = list(base)
        a[pos] = val
        return tuple(a)

    for nc in (1, 2, 4, 6):
        assert fn(*swap(1, L.shape_arr((360, 181, nc))), None) == -22 and "3 components" in L.last_error()
    bad = [swap(0, None), swap(0, C.byref(bad_wcs)), swap(1, None), swap(1, L.shape_arr((0, 181, 3))), swap(4, -1)]
    bad += [swap(p, None) for p in (2, 3, 5, 6, 7, 8)]                                           # a null pointer with n > 0
    bad += [swap(5, P_(sky, 8), swap(4, n - 1)), swap(6, P_(resp, 8), swap(4, n - 1))]            # a 2xN batch not 16-byte aligned
    bad += [swap(4, 2 ** 60), swap(1, L.shape_arr((2 ** 31, 2 ** 31, 3)))]                        # byte counts overflow
    bad += [swap(3, P_(rhs)), swap(3, P_(rhs, 8 * 2 * npl)), swap(2, P_(wts, 8 * 5 * npl))]       # rhs3 and weights6 overlap
    for pos in (5, 6, 7, 8):                                                                     # a map overlaps an input
        bad += [swap(pos, P_(rhs, 16 * 3000)), swap(pos, P_(wts, 16 * 3000 + 8 * 5 * npl))]
    for a in bad:
        assert fn(*a, None) == -22, a
        assert L.last_error()
    # the four other entries: a bad window, shape[2] != 3 for the polarised ones, a bad mode, null pointers with n > 0, overlaps
    s_args = (W, shp, P_(src), 0, 181, n, P_(sky), P_(out))
    t_args = (W, shp, P_(rhs), 0, 181, n, P_(sky), P_(out))
    sp_args = (W, shp, P_(src), 0, 181, n, P_(sky), P_(resp), P_(out))
    tp_args = (W, shp, P_(rhs), 0, 181, n, P_(sky), P_(resp), P_(d), 0)
    entries = ((lib.pxl_sample_car_nearest_f64, s_args, (2, 6, 7)), (lib.pxl_scatter_car_nearest_f64, t_args, (2, 6, 7)),
               (lib.pxl_sample_car_pol_nearest_f64, sp_args, (2, 6, 7, 8)), (lib.pxl_scatter_car_pol_nearest_f64, tp_args, (2, 6, 7, 8)))
    for f, args, ptrs in entries:
        for window in ((-1, 10), (0, 182), (180, 2), (5, -1)):
            assert f(*swap(4, window[1], swap(3, window[0], args)), None) == -22 and "window" in L.last_error()
        for p in ptrs:
            assert f(*swap(p, None, args), None) == -22
        assert f(*swap(0, None, args), None) == -22 and f(*swap(5, -1, args), None) == -22
        assert f(*swap(6, P_(sky, 8), swap(5, n - 1, args)), None) == -22 and "aligned" in L.last_error()
    for f, args in ((lib.pxl_sample_car_pol_nearest_f64, sp_args), (lib.pxl_scatter_car_pol_nearest_f64, tp_args)):
        for nc in (1, 2, 4):
            assert f(*swap(1, L.shape_arr((360, 181, nc)), args), None) == -22 and "3 components" in L.last_error()
    for mode in (-1, 2):
        assert lib.pxl_scatter_car_pol_nearest_f64(*swap(9, mode, tp_args), None) == -22 and "mode" in L.last_error()
    assert lib.pxl_scatter_car_nearest_f64(*swap(6, P_(rhs, 16 * 3000), t_args), None) == -22          # dst overlaps the points
    assert lib.pxl_scatter_car_nearest_f64(*swap(7, P_(rhs, 8 * 1000), t_args), None) == -22           # dst overlaps the values
    for pos in (6, 7, 8):
        assert lib.pxl_scatter_car_pol_nearest_f64(*swap(pos, P_(rhs, 16 * 3000), tp_args), None) == -22
    torch.cuda.synchronize()
    for t, v in ((rhs, -3.5), (wts, 2.5), (src, 1.25), (sky, 0.25), (resp, 0.75), (d, 2.0), (w, 1.5), (out, 9.0)):
        assert bool((t == v).all()), "a refused call wrote"
    # n = 0 succeeds and writes nothing, with null pointers too
    assert fn(W, shp, None, None, 0, None, None, None, None, None) == 0 and fn(*swap(4, 0), None) == 0
    assert lib.pxl_sample_car_nearest_f64(W, shp, None, 0, 181, 0, None, None, None) == 0
    assert lib.pxl_scatter_car_nearest_f64(W, shp, None, 0, 181, 0, None, None, None) == 0
    assert lib.pxl_sample_car_pol_nearest_f64(W, shp, None, 0, 181, 0, None, None, None, None) == 0
    assert lib.pxl_scatter_car_pol_nearest_f64(W, shp, None, 0, 181, 0, None, None, None, 1, None) == 0
    assert lib.pxl_scatter_car_nearest_f64(*swap(4, 0, swap(2, None, t_args)), None) == 0             # nrows = 0: no map needed
    torch.cuda.synchronize()
    assert bool((rhs == -3.5).all()) and bool((wts == 2.5).all())
    # and the valid call does its work, on an explicit stream: all points in one pixel, nine planes
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    assert fn(*good, C.c_void_p(side.cuda_stream)) == 0, L.last_error()
    side.synchronize()
    assert int((rhs != -3.5).sum()) == 3 and int((wts != 2.5).sum()) == 6 and bool((rhs[3] == -3.5).all()) and bool((wts[6] == 2.5).all())
    v = 1.5 * 2.0
    want_r = np.array([v, 0.75 * v, 0.75 * v]) * n - 3.5
    want_w = np.array([1.5, 0.75 * 1.5, 0.75 * 1.5, 0.75 * (0.75 * 1.5), 0.75 * (0.75 * 1.5), 0.75 * (0.75 * 1.5)]) * n + 2.5
    hit = torch.nonzero(rhs[0] != -3.5)[0]
    assert np.allclose(rhs[:3, hit[0], hit[1]].cpu().numpy(), want_r, rtol=1e-12)
    assert np.allclose(wts[:6, hit[0], hit[1]].cpu().numpy(), want_w, rtol=1e-12)


def test_wrapper_refusals(pj, dev):
    """What the Python layer refuses on device tensors before the library is reached."""
    shape, wcs = N.geometries(pj)["box_80x40"]
    f64 = dict(dtype=torch.float64, device=dev)
    sky, resp, d, w = torch.zeros((100, 2), **f64), torch.ones((100, 2), **f64), torch.ones(100, **f64), torch.ones(100, **f64)
    with pytest.raises(ValueError, match="one value per point"):
        pj.scatter_pol_nearest(torch.zeros((3, 100), **f64), sky, resp, shape, wcs)
    with pytest.raises(ValueError, match="d and w must be"):
        pj.bin_pol_nearest(d, torch.ones(99, **f64), sky, resp, shape, wcs)
    with pytest.raises(ValueError, match="resp must be"):
        pj.bin_pol_nearest(d, w, sky, resp[:50], shape, wcs)
    with pytest.raises(ValueError, match="coordinate batches"):
        pj.bin_pol_nearest(d, w, sky[:50], resp[:50], shape, wcs)
    with pytest.raises(ValueError, match="out must be a"):
        pj.bin_pol_nearest(d, w, sky, resp, shape, wcs, rhs=torch.zeros((6, 40, 80), **f64))
    with pytest.raises(ValueError, match="out must be a"):
        pj.bin_pol_nearest(d, w, sky, resp, shape, wcs, weights=torch.zeros((3, 40, 80), **f64))
    with pytest.raises(ValueError, match="Float64 maps"):
        pj.bin_pol_nearest(d, w, sky, resp, shape, wcs, rhs=torch.zeros((3, 40, 80), dtype=torch.float32, device=dev))
    big = torch.zeros((9, 40, 80), **f64)
    with pytest.raises(ValueError, match="may not overlap"):
        pj.bin_pol_nearest(d, w, sky, resp, shape, wcs, rhs=big[:3], weights=big[2:8])
    with pytest.raises(ValueError, match="may not overlap"):
        pj.bin_pol_nearest(big.view(-1)[:100], w, sky, resp, shape, wcs, rhs=big[:3])
    with pytest.raises(ValueError, match="the map's data"):
        pj.sample_nearest(pj.Enmap(torch.zeros((3, 10, 80), **f64), wcs), sky, src_rows=(0, 20), full_shape=shape)
    with pytest.raises(ValueError, match="out overlaps resp"):
        pj.scatter_pol_nearest(d, sky, big.view(-1)[:200].view(100, 2), shape, wcs, out=big[:3])
    with pytest.raises(ValueError, match="not finite"):
        pj.binned_map_pol_nearest([(d * float("nan"), w, sky, resp)], shape, wcs)
    assert not big.any()
