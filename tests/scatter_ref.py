"""numpy yardstick for the scatter-add (pxl_scatter_car_bilinear_f64 / pj.scatter_bilinear), CPU only.

Definition: for point k, (x, y) is the oracle's batched sky2pix(safe=True) in the reciprocal form -- the device is bit-exact
with it, so cells, fractions and every contribution (wy_b * wx_a) * v are identical bits on both sides.  What differs is the
ORDER in which the contributions to one pixel are added: np.add.at here, arrival order of the atomics on the device.  Two
summation orders of the same k terms (the pixel's initial value counted as one) are each within (k - 1) * 2^-53 * S of the exact
sum, S = sum |term|, so they differ by less than

    bound = k * 2^-52 * S        per pixel,

derived, not measured.  scatter() returns (ref, k, S); held() applies the bound to every pixel.  tests/test_scatter_ref.py
holds this file to oracle.sample_bilinear (adjoint identity, and tap by tap on one-hot maps)."""
import numpy as np

from conftest import DEG

CELL_LIMIT = 1073741824.0          # split_cell's clamp (pxl_device.h): a cell that far out has no tap on any map


def taps(O, wcs, shape, sky, row0=0, nrows=None):
    """Per point and tap (a, b) in the order (0,0), (1,0), (0,1), (1,1): flat index into the resident (nrows, nx) plane, or -1
    for a dropped tap, and the weight wy_b * wx_a.  Returns (idx (N, 4) int64, w (N, 4) float64)."""
    nx, ny = int(shape[0]), int(shape[1])
    nrows = ny - row0 if nrows is None else nrows
    sky = np.ascontiguousarray(sky, dtype=np.float64).reshape(-1, 2)
    n = sky.shape[0]
    if n == 0:
        return np.zeros((0, 4), np.int64), np.zeros((0, 4))
    pix = O.sky2pix(wcs, (nx, ny), sky, safe=True)
    x, y = pix[:, 0], pix[:, 1]
    fin = np.isfinite(x) & np.isfinite(y)
    xs, ys = np.where(fin, x, 0.0), np.where(fin, y, 0.0)
    flx, fly = np.floor(xs), np.floor(ys)
    fx, fy = xs - flx, ys - fly
    i0 = np.clip(flx, -CELL_LIMIT, CELL_LIMIT).astype(np.int64)
    j0 = np.clip(fly, -CELL_LIMIT, CELL_LIMIT).astype(np.int64)
    periodic = O.is_periodic(wcs, nx)
    idx = np.empty((n, 4), np.int64)
    w = np.empty((n, 4))
    wx, wy = (1 - fx, fx), (1 - fy, fy)
    for t, (a, b) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        i, j = i0 + a, j0 + b
        if periodic:
            col_ok = np.ones(n, bool)
            i = (i - 1) % nx + 1
        else:
            col_ok = (i >= 1) & (i <= nx)
        jr = j - 1 - row0
        ok = fin & col_ok & (j >= 1) & (j <= ny) & (jr >= 0) & (jr < nrows)
        idx[:, t] = np.where(ok, jr * nx + (i - 1), -1)
        w[:, t] = wy[b] * wx[a]
    return idx, w


def to_window(idx, nx, row0, nrows, what="tap"):
    """Flat indices into the full (ny, nx) plane (-1: no tap) -> flat indices into the resident rows [row0, row0 + nrows).  A tap
    that is on the map but outside the window RAISES: the banded yardsticks built on this never drop one silently."""
    idx = np.asarray(idx, dtype=np.int64)
    on = idx >= 0
    row = idx // int(nx)
    bad = on & ((row < row0) | (row >= row0 + nrows))
    if bad.any():
        raise ValueError("%s: %d taps on rows %d .. %d, outside the resident rows [%d, %d)"
                         % (what, int(bad.sum()), int(row[bad].min()), int(row[bad].max()), row0, row0 + nrows))
    return np.where(on, idx - int(row0) * int(nx), -1)


def window_rows(shape, row0, nrows):
    """(row0, nrows, windowed): the resident rows, the whole map when nrows is None and row0 is 0."""
    ny = int(shape[1])
    return int(row0), (ny - int(row0) if nrows is None else int(nrows)), not (row0 == 0 and nrows in (None, ny))


def require_inside(O, wcs, shape, sky, row0, nrows, what="bilinear tap"):
    """Raise unless every tap of every point lies on the resident rows or off the map altogether (taps() itself DROPS a tap that
    is on the map but outside the window, which is the device's window rule and not what a banded yardstick wants)."""
    to_window(taps(O, wcs, shape, sky)[0], int(shape[0]), row0, nrows, what)


def scatter(O, wcs, shape, sky, vals, out=None, row0=0, nrows=None):
    """vals (nc, N) or (N,); out: initial (nc, nrows, nx) map or None (zeros, not counted as a term).
    Returns (ref, k, S), each (nc, nrows, nx): the np.add.at sum, the number of terms and the sum of |term| per pixel, an
    initial `out` counted as one term."""
    nx, ny = int(shape[0]), int(shape[1])
    nrows = ny - row0 if nrows is None else nrows
    vals = np.atleast_2d(np.asarray(vals, dtype=np.float64))
    nc = vals.shape[0]
    if out is None:
        ref = np.zeros((nc, nrows * nx))
        k = np.zeros((nc, nrows * nx), np.int64)
    else:
        ref = np.array(out, dtype=np.float64).reshape(nc, nrows * nx).copy()
        k = np.ones((nc, nrows * nx), np.int64)
    S = np.abs(ref)
    idx, w = taps(O, wcs, shape, sky, row0, nrows)
    for t in range(4):
        on = idx[:, t] >= 0
        at = idx[on, t]
        for c in range(nc):
            term = w[on, t] * vals[c, on]
            np.add.at(ref[c], at, term)
            np.add.at(S[c], at, np.abs(term))
            np.add.at(k[c], at, 1)
    sh = (nc, nrows, nx)
    return ref.reshape(sh), k.reshape(sh), S.reshape(sh)


def bound(k, S):
    return k * 2.0 ** -52 * S


def held(got, ref, k, S, what=""):
    """Every pixel of got within bound of ref; NaN exactly where ref is NaN.  Prints and returns the worst error / bound."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN pixels differ by position"
    with np.errstate(invalid="ignore"):
        err = np.where(nan, 0.0, np.abs(got - ref))
        b = np.where(nan, 0.0, bound(k, S))
    assert np.all(err <= b), "%s: %d pixels beyond k * 2^-52 * S (worst excess %g)" % (what, int((err > b).sum()), float((err - b).max()))
    ratio = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print("%s: worst error / bound = %.3g over %d pixels, max k = %d" % (what, ratio, err.size, int(k.max())))
    return ratio


def geometries(pj):
    """name -> (shape, wcs): the 1 degree full sky (periodic), the reference's 0.5 degree box, the 360/1024 degree full sky."""
    return {"cc_360x181": pj.fullsky_geometry(1.0 * DEG),
            "box_80x40": pj.geometry([[20 * DEG, -20 * DEG], [-10 * DEG, 10 * DEG]], 0.5 * DEG),
            "cc_1024x513": pj.fullsky_geometry(2 * np.pi / 1024)}


def sphere_points(n, seed):
    """Uniform on the sphere, (n, 2) of (ra, dec)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-np.pi, np.pi, n), np.arcsin(rng.uniform(-1, 1, n))], axis=1)


def box_points(O, wcs, shape, n, seed, margin=1.5):
    """Points spread over the map's pixel range widened by `margin` pixels on every side: (n, 2) of (ra, dec)."""
    rng = np.random.default_rng(seed)
    pix = np.stack([rng.uniform(1 - margin, shape[0] + margin, n), rng.uniform(1 - margin, shape[1] + margin, n)], axis=1)
    return O.pix2sky(wcs, pix, O.WRAP_NONE)


def adjoint_gap(m, pm, d, ref, k, S):
    """|<P m, d> - <m, P^T d>| and its bound 2^-53 * sum_p |m_p| * S_p * (8 + 2 k_p), dot products in longdouble.
    The 8 covers the sampler's three nested lerps (2 roundings each for the row lerps of one tap's path, 2 for the column lerp,
    against the 2 of the product weight and 1 of the term, and as many again on the other side); 2 k_p the summation."""
    L = np.longdouble
    lhs = np.sum(pm.astype(L) * np.atleast_2d(d).astype(L))
    rhs = np.sum(m.reshape(ref.shape).astype(L) * ref.astype(L))
    b = 2.0 ** -53 * np.sum(np.abs(m.reshape(ref.shape)).astype(L) * S.astype(L) * (8 + 2 * k).astype(L))
    return float(abs(lhs - rhs)), float(b)
