"""Yardstick of the cubic B-spline path, numpy only, no device.

The definition, for a plane m of shape (nx, ny) held as a C-order (ny, nx) array:

  coefficients  (b[i-1,j] + 4 b[i,j] + b[i+1,j]) / 6 = m[i,j] along RA, then the same system along DEC on b.  Along RA the
                system is cyclic iff the map is periodic; otherwise, and always along DEC, whole-sample mirror
                (c[0] = c[2], c[n+1] = c[n-1]).  Solved here DIRECTLY: a tridiagonal elimination (Thomas), with the
                Sherman-Morrison correction for the cyclic corner terms -- not the pole recursion the kernel runs.
  evaluation    i0 = floor(x), f = x - i0, taps i0-1 .. i0+2, weights (1-f)^3/6, (3f^3-6f^2+4)/6, (-3f^3+3f^2+3f+1)/6, f^3/6;
                the RA sum of each tap row first, each sum left to right.  Tap indices wrap on a periodic RA axis and are
                mirrored otherwise.  0 where y is outside [0.5, ny+0.5] or, on a non-periodic map, x outside [0.5, nx+0.5].

Everything takes a dtype: np.float64 is the yardstick the device is compared with, np.longdouble (x87 80-bit) measures the
yardstick's own rounding error, from which the device's allowance is derived (K below).  Positions (xs, ys) are always
Float64: they come from oracle.reproject_tables / oracle.sky2pix(safe=True), so coordinate parity is the existing oracle's."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)

# Worst |Float64 yardstick - long-double yardstick| in units of eps * max|plane|, measured on the inputs of
# tests/test_gpu_spline.py: every geometry and input kind of the prefilter test, every launch-path size, the 8192 x 4097 map
# (5.29), every reprojection case, the identity cases and 1e6 uniform sphere points (from numpy's generator, not the
# device's).  tests/test_spline_ref.py::test_k_was_measured repeats the measurement, the 8192 x 4097 map excepted.
#   prefilter coefficients   6.061 (cc_1024x513, normal)
#   interpolated values      3.541 (the 1e6 points; Float64 prefilter + evaluation against both in long double)
# The device sums in the same order as evaluate(), but runs the prefilter as a pole recursion from a 32-sample warm-up
# (5e-19 relative) where this file eliminates; neither is worth more than a small factor: it is allowed 4 x the larger.
# (A numpy restatement of the kernel's recursion measured 6.08 in the same units.)
MEASURED_WORST_PREFILTER = 6.07
MEASURED_WORST_EVALUATE = 3.55
K = 4.0 * max(MEASURED_WORST_PREFILTER, MEASURED_WORST_EVALUATE)


def bound(m):
    """Per-value error allowed on anything computed from the plane(s) m: K * eps * max|plane|, one number per plane."""
    m = np.asarray(m, dtype=np.float64)
    planes = m.reshape((-1,) + m.shape[-2:])
    return np.array([K * EPS * float(np.abs(p).max()) for p in planes])


# ---- the two systems --------------------------------------------------------------------------------------------------
def _thomas(lower, diag, upper, rhs):
    """Tridiagonal elimination along axis 0 of rhs (n, L); lower[0] and upper[-1] are ignored."""
    n = rhs.shape[0]
    cp = np.empty(n, dtype=rhs.dtype)
    d = np.empty_like(rhs)
    cp[0] = upper[0] / diag[0]
    d[0] = rhs[0] / diag[0]
    for k in range(1, n):
        den = diag[k] - lower[k] * cp[k - 1]
        cp[k] = upper[k] / den
        d[k] = (rhs[k] - lower[k] * d[k - 1]) / den
    for k in range(n - 2, -1, -1):
        d[k] = d[k] - cp[k] * d[k + 1]
    return d


def solve_axis0(m, cyclic, dtype=np.float64):
    """c with (c[k-1] + 4 c[k] + c[k+1]) / 6 = m[k] along axis 0 of the (n, L) array m."""
    m = np.asarray(m, dtype=dtype)
    n = m.shape[0]
    assert n >= 4
    one, four, six = dtype(1), dtype(4), dtype(6)
    rhs = six * m
    lower = np.full(n, one, dtype=dtype); diag = np.full(n, four, dtype=dtype); upper = np.full(n, one, dtype=dtype)
    if not cyclic:
        upper[0] = dtype(2); lower[n - 1] = dtype(2)          # c[0] = c[2], c[n+1] = c[n-1]
        return _thomas(lower, diag, upper, rhs)
    # cyclic: A = B + u v^T with u = (g, 0, .., 0, 1), v = (1, 0, .., 0, 1/g), g = -4
    g = -four
    diag[0] = four - g
    diag[n - 1] = four - one / g
    u = np.zeros((n, 1), dtype=dtype); u[0, 0] = g; u[n - 1, 0] = one
    y = _thomas(lower, diag, upper, rhs)
    q = _thomas(lower, diag, upper, u)
    vy = y[0] + y[n - 1] / g
    vq = q[0, 0] + q[n - 1, 0] / g
    return y - q * (vy / (one + vq))[None, :]


def prefilter(m, periodic, dtype=np.float64):
    """m: (ny, nx) or (nc, ny, nx).  RA first (axis -1), then DEC (axis -2)."""
    m = np.asarray(m)
    if m.ndim == 3:
        return np.stack([prefilter(p, periodic, dtype) for p in m])
    b = solve_axis0(np.ascontiguousarray(m.T), bool(periodic), dtype).T          # along RA
    return np.ascontiguousarray(solve_axis0(np.ascontiguousarray(b), False, dtype))   # along DEC


def residual(c, m, periodic):
    """max |system(c) - m| of both axes applied in turn (DEC system first undoes the DEC solve), in long double."""
    c = np.asarray(c, dtype=np.longdouble)
    up = np.vstack([c[1:2], c[:-1]]); dn = np.vstack([c[1:], c[-2:-1]])
    b = (up + 4 * c + dn) / 6
    if periodic:
        lf = np.roll(b, 1, axis=1); rt = np.roll(b, -1, axis=1)
    else:
        lf = np.hstack([b[:, 1:2], b[:, :-1]]); rt = np.hstack([b[:, 1:], b[:, -2:-1]])
    return float(np.abs((lf + 4 * b + rt) / 6 - np.asarray(m, dtype=np.longdouble)).max())


# ---- evaluation -------------------------------------------------------------------------------------------------------
def fold(t, n, periodic):
    """Any integer position (1-based) -> [1, n]: modulo n, or the whole-sample mirror applied as often as needed."""
    t = np.asarray(t, dtype=np.int64)
    if periodic:
        return (t - 1) % n + 1
    p = 2 * n - 2
    u = (t - 1) % p
    return np.where(u >= n, p - u, u) + 1


def weights(f, dtype=np.float64):
    f = np.asarray(f, dtype=dtype)
    t = dtype(1) - f
    f2 = f * f
    f3 = f2 * f
    return [((t * t) * t) / dtype(6), ((dtype(3) * f3 - dtype(6) * f2) + dtype(4)) / dtype(6),
            (((dtype(-3) * f3 + dtype(3) * f2) + dtype(3) * f) + dtype(1)) / dtype(6), f3 / dtype(6)]


def _split(x):
    x = np.asarray(x, dtype=np.float64)
    i0 = np.floor(x)
    return i0.astype(np.int64), x - i0


def in_domain(x, n):
    x = np.asarray(x, dtype=np.float64)
    return (x >= 0.5) & (x <= n + 0.5)


def evaluate(c, xs, ys, periodic, dtype=np.float64):
    """Separable evaluation: c (ny, nx) or (nc, ny, nx), xs (nxo,), ys (nyo,) -> (.., nyo, nxo)."""
    c = np.asarray(c)
    if c.ndim == 3:
        return np.stack([evaluate(p, xs, ys, periodic, dtype) for p in c])
    c = c.astype(dtype, copy=False)
    ny, nx = c.shape
    okx = np.ones(len(xs), bool) if periodic else in_domain(xs, nx)
    oky = in_domain(ys, ny)
    i0, fx = _split(np.where(okx, xs, 1.0))
    j0, fy = _split(np.where(oky, ys, 1.0))
    wx, wy = weights(fx, dtype), weights(fy, dtype)
    cols = [fold(i0 - 1 + a, nx, periodic) - 1 for a in range(4)]
    out = None
    for b in range(4):
        rows = c[fold(j0 - 1 + b, ny, False) - 1]                     # (nyo, nx)
        h = wx[0][None, :] * rows[:, cols[0]]
        for a in range(1, 4):
            h = h + wx[a][None, :] * rows[:, cols[a]]
        out = wy[b][:, None] * h if out is None else out + wy[b][:, None] * h
    out = np.where(oky[:, None] & okx[None, :], out, dtype(0))
    return out


def evaluate_points(c, x, y, periodic, dtype=np.float64, row0=0, ny=None):
    """Scattered evaluation: c (ny, nx) or (nc, ny, nx), x, y (n,) -> (.., n).  With ny given, c holds only the coefficient
    rows [row0, row0 + c.shape[-2]) of a map of ny rows: x, y, the domain and the folds are the full map's, and a tap row of a
    point inside the domain that folds or falls outside the resident rows raises."""
    c = np.asarray(c)
    if c.ndim == 3:
        return np.stack([evaluate_points(p, x, y, periodic, dtype, row0, ny) for p in c])
    c = c.astype(dtype, copy=False)
    nrows, nx = c.shape
    ny = nrows if ny is None else int(ny)
    assert 0 <= row0 and row0 + nrows <= ny
    ok = in_domain(y, ny) & (np.ones(len(x), bool) if periodic else in_domain(x, nx))
    i0, fx = _split(np.where(ok, x, 1.0))
    j0, fy = _split(np.where(ok, y, 1.0))
    wx, wy = weights(fx, dtype), weights(fy, dtype)
    cols = [fold(i0 - 1 + a, nx, periodic) - 1 for a in range(4)]
    out = None
    for b in range(4):
        r = fold(j0 - 1 + b, ny, False) - 1 - row0
        outside = ok & ((r < 0) | (r >= nrows))
        if outside.any():
            raise ValueError("cubic tap: %d tap rows outside the resident rows [%d, %d)" % (int(outside.sum()), row0, row0 + nrows))
        r = np.where(ok, r, 0)
        h = wx[0] * c[r, cols[0]]
        for a in range(1, 4):
            h = h + wx[a] * c[r, cols[a]]
        out = wy[b] * h if out is None else out + wy[b] * h
    return np.where(ok, out, dtype(0))


def worst_ratio(got, ref, m):
    """max |got - ref| / bound over every value, planes held to their own bound."""
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    g = got.reshape((len(bound(m)), -1)); r = ref.reshape(g.shape)
    return float((np.abs(g - r).max(axis=1) / bound(m)).max())


# ---- the inputs of the GPU tests (shared with the measurement of K) ------------------------------------------------------
DEG = np.pi / 180


def geometries(pj):
    """name -> (shape, wcs): full-sky CC at 1 degree and 360/1024 degree, Fejer1 full sky, the reference's 0.5 degree box."""
    import tap_ref
    return tap_ref.geometries(pj, ("cc_360x181", "cc_1024x513", "fejer1_360x180", "box_80x40"))


def input_map(kind, shape, seed, nc=3):
    """(nc, ny, nx) test input: 'normal', 'spikes' (single spikes next to each edge and on the seam columns), 'constant'."""
    nx, ny = int(shape[0]), int(shape[1])
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.normal(size=(nc, ny, nx))
    if kind == "constant":
        return np.full((nc, ny, nx), 2.5) * np.arange(1, nc + 1)[:, None, None]
    m = np.zeros((nc, ny, nx))
    spots = [(0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1), (1, nx // 2), (ny - 2, nx // 3), (ny // 2, 0), (ny // 3, nx - 1),
             (ny // 2, 1), (ny // 2 + 5, nx - 2)]
    for c in range(nc):
        j, i = spots[c % len(spots)]
        m[c, j, i] = 1.0 + c
        j, i = spots[(c + 4) % len(spots)]
        m[c, j, i] = -2.0
        j, i = spots[(c + 6) % len(spots)]
        m[c, j, i] += 3.0
    return m


def shifted(wcs, dx=0.0, dy=0.0, scale=1):
    """The grid `scale` times finer than wcs whose pixel (1, 1) centre sits dx, dy SOURCE pixels from wcs's (1, 1) centre."""
    cd = (wcs.cdelt[0] / scale, wcs.cdelt[1] / scale)
    cp = (scale * (wcs.crpix[0] - 1 - dx) + 1, scale * (wcs.crpix[1] - 1 - dy) + 1)
    return type(wcs)(cd, cp, wcs.crval)


def reproject_cases(pj):
    """name -> ((shape_in, wcs_in), (shape_out, wcs_out)) of test_gpu_spline.py's reprojections."""
    g = geometries(pj)
    (s1, w1) = g["cc_360x181"]
    cases = {}
    cases["refine_2x"] = ((s1, w1), pj.fullsky_geometry(0.5 * DEG))
    cases["half_pixel_shift"] = ((s1, w1), (s1, shifted(w1, 0.5, 0.5)))
    sub = pj.slice_geometry(s1, w1, (100, 200), (50, 120))
    cases["sub_box_onto_full_sky"] = (sub, (s1, w1))
    cases["box_refined_with_margin"] = (g["box_80x40"], ((200, 120), shifted(g["box_80x40"][1], -10.25, -10.25, 2)))
    cases["cc_to_fejer1"] = ((s1, w1), g["fejer1_360x180"])
    return cases


def sphere_points(n, seed):
    """Uniform points on the sphere as (n, 2) (ra, dec), the distribution of pxl_fill_sphere_points_f64."""
    rng = np.random.default_rng(seed)
    return np.stack([2 * np.pi * rng.random(n) - np.pi, np.arcsin(2 * rng.random(n) - 1)], axis=1)


# sizes of test_gpu_spline.py::test_prefilter_launch_paths (PXL_SPL_WARM, PXL_SPL_SEG, PXL_SPL_LINES of pxl_spline.h)
WARM, SEG, LINES = 32, 256, 16
LAUNCH_SIZES = [(4, 4), (5, 7), (WARM - 1, WARM + 1), (WARM, WARM - 1), (WARM + 1, WARM), (SEG - 1, LINES + 1), (SEG, LINES),
                (SEG + 1, LINES - 1), (LINES + 1, SEG - 1), (LINES, SEG), (LINES - 1, SEG + 1), (SEG + WARM, 9),
                (SEG + WARM + 1, 11), (9, SEG + WARM + 1), (333, 17), (2 * SEG + 3, 2 * SEG + 5), (10, 10), (7, 300)]


def launch_geometry(pj, nx, ny, periodic):
    """An nx x ny CAR grid: RA spanning the full circle (periodic) or 3/4 of it, DEC spanning +-60 degrees."""
    span = 2 * np.pi if periodic else 1.5 * np.pi
    cd = (-(span / nx) / DEG, (120.0 / ny))
    return (nx, ny), pj.CarClenshawCurtis(cd, (nx / 2 + 0.5, ny / 2 + 0.5), (0.0, 0.0))


def launch_input(shape):
    nx, ny = shape
    m = input_map("normal", shape, seed=nx * 1000 + ny, nc=2)
    m[0, 0, 0] = 5.0
    m[1, ny - 1, nx - 1] = -5.0
    return m
