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

import tap_ref


def taps(O, wcs, shape, sky, row0=0, nrows=None):
    """Per point and tap (a, b) in the order (0,0), (1,0), (0,1), (1,1): flat index into the resident (nrows, nx) plane, or -1
    for a dropped tap, and the weight wy_b * wx_a.  Returns (idx (N, 4) int64, w (N, 4) float64)."""
    fin, _x, _y, i0, j0, fx, fy = tap_ref.position(O, wcs, shape, sky)
    periodic = O.is_periodic(wcs, int(shape[0]))
    wx, wy = (1 - fx, fx), (1 - fy, fy)
    order = ((0, 0), (1, 0), (0, 1), (1, 1))
    idx = np.stack([tap_ref.flat_index(i0 + a, j0 + b, fin, shape, periodic) for a, b in order], axis=1)
    w = np.stack([wy[b] * wx[a] for a, b in order], axis=1)
    return tap_ref.window(idx, shape, row0, nrows, "drop"), w


def scatter(O, wcs, shape, sky, vals, out=None, row0=0, nrows=None):
    """vals (nc, N) or (N,); out: initial (nc, nrows, nx) map or None (zeros, not counted as a term).
    Returns (ref, k, S), each (nc, nrows, nx): the np.add.at sum, the number of terms and the sum of |term| per pixel, an
    initial `out` counted as one term (tap_ref.accumulate)."""
    nx, nrows = int(shape[0]), tap_ref.rows(shape, row0, nrows)[1]
    idx, w = taps(O, wcs, shape, sky, row0, nrows)
    return tuple(a.reshape(len(a), nrows, nx) for a in tap_ref.accumulate(idx, w, vals, nrows * nx, out))


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
    return tap_ref.geometries(pj, ("cc_360x181", "box_80x40", "cc_1024x513"))


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
    return tap_ref.adjoint_gap(m, pm, d, ref, S, 8 + 2 * k)
