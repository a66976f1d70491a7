"""numpy yardstick for the transpose of the order-3 sampler, CPU only: E^T, the sixteen-tap scatter-add
(pxl_scatter_car_cubic_f64 / pj.scatter_cubic), and F^T, the transposed prefilter (pxl_spline_prefilter_transpose_car_f64 /
pj.spline_prefilter_transpose).  The sampler is P = E F, so P^T = F^T E^T (pj.scatter(order=3)).

E^T.  For point k, (x, y) is the oracle's batched sky2pix(safe=True) in the reciprocal form; cell, fractions, domain rule,
weights and folded taps are spline_ref's (fold / weights / in_domain), which the device restates op for op, so every
contribution (wy[b] * wx[a]) * v is the same bits on both sides.  What differs is the ORDER of the additions into one pixel:
np.add.at here, arrival order of the atomics on the device.  As in scatter_ref, two orders of the same k terms (the pixel's
initial value counted as one) differ by less than k * 2^-52 * S, S = sum |term|: derived, not measured.  scatter() returns
(ref, k, S) and scatter_ref.held() applies the bound.

F^T.  A direct Thomas elimination of the TRANSPOSED systems, RA first, then DEC (the device's order).  The mirrored system has
upper[0] = lower[n-1] = 2; its transpose has lower[1] = upper[n-2] = 2 instead.  The cyclic system is symmetric.  This is not
D prefilter D^-1 (D = diag(1/2, 1, .., 1, 1/2) along every mirrored axis), which is what the device runs: the identity
B^-T = D B^-1 D^-1 is under test.  tests/test_scatter_cubic_ref.py holds this file to dense solves, to that identity, to the
adjoint identity against spline_ref and to one-hot maps."""
import numpy as np

import scatter_ref
import spline_ref
import tap_ref

EPS = spline_ref.EPS

# Worst |Float64 F^T yardstick - long-double F^T yardstick| in units of eps * max|plane of D^-1 g|, measured on the inputs of
# tests/test_gpu_scatter_cubic.py (ft_inputs() below: every launch-path size, periodic and not; 1024 x 513 with three
# components; the periodic map of equal rows; the composite cases' E^T maps; the NaN case with its NaN taken out).
# tests/test_scatter_cubic_ref.py::test_kt_was_measured repeats the measurement.
#   worst 3.759 (cc_1024x513, three components); the boxes 0.2 .. 1.2, the periodic launch sizes 1.1 .. 2.4
# The device runs spline_ref's prefilter recursion between two exact scalings where this file eliminates the transposed
# system; as for spline_ref.K it is allowed 4 x the yardstick's own error.
MEASURED_WORST_FT = 3.76
KT = 4.0 * MEASURED_WORST_FT


# ---- E^T ----------------------------------------------------------------------------------------------------------------
def taps(O, wcs, shape, sky, row0=0, nrows=None):
    """Per point and tap, b (row) outer, a (column) inner: flat index into the resident (nrows, nx) plane, or -1 for every tap of
    a point that is not live (position not finite, or outside the domain), and the weight wy[b] * wx[a].  Positions, folds and
    the domain are those of the FULL (ny, nx) map; a live tap that folds or falls outside the resident rows raises
    (tap_ref.window's rule "raise").  The position is tap_ref.position's; cell, fractions and the rest are spline_ref's.
    Returns (idx (N, 16) int64, w (N, 16) float64)."""
    nx, ny = int(shape[0]), int(shape[1])
    fin, x, y = tap_ref.position(O, wcs, shape, sky)[:3]
    n = len(fin)
    periodic = bool(O.is_periodic(wcs, nx))
    xs, ys = np.where(fin, x, 1.0), np.where(fin, y, 1.0)
    live = fin & spline_ref.in_domain(ys, ny) & (np.ones(n, bool) if periodic else spline_ref.in_domain(xs, nx))
    xs, ys = np.where(live, xs, 1.0), np.where(live, ys, 1.0)
    i0, fx = spline_ref._split(xs)
    j0, fy = spline_ref._split(ys)
    wx, wy = spline_ref.weights(fx), spline_ref.weights(fy)
    idx = np.empty((n, 16), np.int64)
    w = np.empty((n, 16))
    for b in range(4):
        row = spline_ref.fold(j0 - 1 + b, ny, False) - 1
        for a in range(4):
            col = spline_ref.fold(i0 - 1 + a, nx, periodic) - 1
            idx[:, 4 * b + a] = np.where(live, row * nx + col, -1)
            w[:, 4 * b + a] = wy[b] * wx[a]
    return tap_ref.window(idx, shape, row0, nrows, "raise", "cubic tap"), w


def scatter(O, wcs, shape, sky, vals, out=None, row0=0, nrows=None):
    """vals (nc, N) or (N,); out: initial (nc, nrows, nx) map or None (zeros, not counted as a term): rows [row0, row0 + nrows)
    of the full map, all of it by default.  Returns (ref, k, S), each (nc, nrows, nx): the np.add.at sum, the number of terms and
    the sum of |term| per pixel, an initial `out` counted as one term."""
    nx, nrows = int(shape[0]), tap_ref.rows(shape, row0, nrows)[1]
    idx, w = taps(O, wcs, shape, sky, row0, nrows)
    return tuple(a.reshape(len(a), nrows, nx) for a in tap_ref.accumulate(idx, w, vals, nrows * nx, out, bincount=True))


def nonzero_terms(O, wcs, shape, sky, vals):
    """(nc, ny, nx): how many of a pixel's terms are not zero (NaN counts).  A pixel with at most one is added to once at most,
    whatever the order, so the device must give the yardstick's bits there."""
    nx, ny = int(shape[0]), int(shape[1])
    idx, w = taps(O, wcs, shape, sky)
    nz = tap_ref.nonzero_terms(idx, w, vals, ny * nx)
    return nz.reshape(len(nz), ny, nx)


# ---- F^T ----------------------------------------------------------------------------------------------------------------
def solve_axis0_transpose(g, cyclic, dtype=np.float64):
    """c with B^T c = g along axis 0 of the (n, L) array g, B the system of spline_ref.solve_axis0."""
    if cyclic:
        return spline_ref.solve_axis0(g, True, dtype)                 # the cyclic system is symmetric
    g = np.asarray(g, dtype=dtype)
    n = g.shape[0]
    assert n >= 4
    lower = np.full(n, dtype(1), dtype=dtype); diag = np.full(n, dtype(4), dtype=dtype); upper = np.full(n, dtype(1), dtype=dtype)
    lower[1] = dtype(2); upper[n - 2] = dtype(2)                          # B[0, 1] = B[n-1, n-2] = 2/6, transposed
    return spline_ref._thomas(lower, diag, upper, dtype(6) * g)


def prefilter_transpose(g, periodic, dtype=np.float64):
    """g: (ny, nx) or (nc, ny, nx).  RA first (axis -1), then DEC (axis -2)."""
    g = np.asarray(g)
    if g.ndim == 3:
        return np.stack([prefilter_transpose(p, periodic, dtype) for p in g])
    b = solve_axis0_transpose(np.ascontiguousarray(g.T), bool(periodic), dtype).T
    return np.ascontiguousarray(solve_axis0_transpose(np.ascontiguousarray(b), False, dtype))


def edge_scale(g, periodic, factor):
    """D (factor 0.5) or D^-1 (factor 2) of every mirrored axis: the two edge rows, and the two edge columns unless periodic."""
    g = np.array(g, copy=True)
    g[..., 0, :] *= factor; g[..., -1, :] *= factor
    if not periodic:
        g[..., :, 0] *= factor; g[..., :, -1] *= factor
    return g


def bound_t(g, periodic):
    """Per-value error allowed on F^T g: KT * eps * max|plane of D^-1 g|, one number per plane."""
    s = np.abs(edge_scale(np.asarray(g, dtype=np.float64), periodic, 2.0))
    return np.array([KT * EPS * float(p.max()) for p in s.reshape((-1,) + s.shape[-2:])])


def worst_ratio_t(got, ref, g, periodic):
    """max |got - ref| / bound_t over every value, planes held to their own bound."""
    b = bound_t(g, periodic)
    a = np.asarray(got, dtype=np.float64).reshape(len(b), -1); r = np.asarray(ref, dtype=np.float64).reshape(a.shape)
    return float((np.abs(a - r).max(axis=1) / b).max())


def composite_bound(g, k, S, periodic):
    """Per-plane bound on every pixel of F^T E^T d: 36 * max_p (k_p 2^-52 S_p) + KT eps max|D^-1 g|, g = E^T d (the yardstick's).
    The 36, derived: the device's g is within k 2^-52 S of the yardstick's pixel by pixel; F^T = D F D^-1 per mirrored axis
    amplifies a perturbation's maximum by at most |D|.|B^-1|.|D^-1| = 1 * 3 * 2 per axis (||B^-1||_inf = sqrt(3) (1 + 2|z| /
    (1 - |z|)) = 3 with z = sqrt(3) - 2; doubling the edges at most doubles the maximum, halving them does not raise it), 6 per
    axis, 36 over both."""
    eb = scatter_ref.bound(k, S)
    eb = eb.reshape((-1,) + eb.shape[-2:])
    return 36.0 * np.array([float(p.max()) for p in eb]) + bound_t(g, periodic)


# ---- the inputs of the GPU tests (shared with the measurement of KT) -----------------------------------------------------
def geometries(pj):
    """From tap_ref's table: scatter_ref's geometries plus the two smallest boxes: 4 x 4 (every tap row and column of every point folds) and 5 x 7."""
    return tap_ref.geometries(pj, ("cc_360x181", "box_80x40", "cc_1024x513", "box_4x4", "box_5x7"))


COMPOSITE = ("cc_360x181", "box_80x40", "box_5x7")          # the geometries of the composite and adjoint tests
N_COMPOSITE = 100000


def composite_case(pj, O, geom):
    """-> (shape, wcs, sky (n, 2), d (2, n), m (2, ny, nx)): sphere points plus box points with the 1.5-pixel margin."""
    shape, wcs = geometries(pj)[geom]
    rng = np.random.default_rng(len(geom))
    half = N_COMPOSITE // 2
    if geom.startswith("cc_"):
        sky = np.concatenate([scatter_ref.sphere_points(half, 3), scatter_ref.box_points(O, wcs, shape, half, 4)])
    else:
        sky = scatter_ref.box_points(O, wcs, shape, N_COMPOSITE, 4)
    d = rng.normal(size=(2, sky.shape[0]))
    m = rng.normal(size=(2, shape[1], shape[0]))
    return shape, wcs, sky, d, m


def ft_launch_input(shape):
    """The launch-path input of the F^T tests: spline_ref.launch_input, whose spikes sit on the corners D scales."""
    return spline_ref.launch_input(shape)


def equal_rows_map(shape, seed=17):
    """A map whose rows are all the same: along DEC the transposed solve of a constant column is all that happens."""
    nx, ny = int(shape[0]), int(shape[1])
    return np.tile(np.random.default_rng(seed).normal(size=(1, 1, nx)), (2, ny, 1))


NAN_CASE = ("cc_360x181", (1, 90, 200))          # geometry and (plane, row, column) of the NaN pixel of the non-finite test


def nan_case_map(pj):
    shape, wcs = geometries(pj)[NAN_CASE[0]]
    return shape, wcs, np.random.default_rng(23).normal(size=(2, shape[1], shape[0]))


def ft_inputs(pj, O):
    """Yields (name, g, periodic): every map the GPU tests give to F^T, NaN-free."""
    for nx, ny in spline_ref.LAUNCH_SIZES:
        for per in (True, False):
            yield "launch %d x %d %s" % (nx, ny, "periodic" if per else "box"), ft_launch_input((nx, ny)), per
    yield "cc_1024x513 nc=3", spline_ref.input_map("normal", (1024, 513), seed=31, nc=3), True
    yield "equal rows 360x181", equal_rows_map((360, 181)), True
    for geom in COMPOSITE:
        shape, wcs, sky, d, _m = composite_case(pj, O, geom)
        yield "E^T d " + geom, scatter(O, wcs, shape, sky, d)[0], bool(O.is_periodic(wcs, shape[0]))
    shape, wcs, g = nan_case_map(pj)
    yield "NaN case, NaN taken out", g, True
