"""What the numpy yardsticks of the pointing operators share, CPU only: the position of a point on the map, the flat index of a
pixel, the row window, the (ref, k, S) accumulation, the count of non-zero terms, the matrix of P from the taps, the adjoint
gap and the table of named geometries.  scatter_ref (order 1), nearest_ref (order 0), scatter_cubic_ref (order 3), pol_ref,
normal_ref and destripe_ref are short calls of these, as the device builds its tap geometry once in pxl_taps.h.

Why a module of its own and not scatter_ref.py: scatter_ref is the yardstick of ONE operator, and test_scatter_ref.py holds it
to the oracle's bilinear sampler.  nearest_ref and scatter_cubic_ref imported scatter_ref for its clamp, its window and its
geometries, and each other for theirs, in a ring; with the shared layer below all of them every yardstick imports downwards only,
and the next operator's yardstick starts from this file without reading another operator's.

One difference is kept, not forced: scatter_cubic_ref forms S with np.bincount (the tap's magnitudes summed from zero, then added
to S), scatter_ref and nearest_ref with np.add.at (added to S one by one).  The two associate differently and so differ in the
last bits of S; accumulate() takes the form as `bincount`.  k is an integer count and ref is np.add.at in all three."""
import numpy as np

from conftest import DEG

CELL_LIMIT = 1073741824.0          # split_cell's clamp (pxl_device.h): a cell that far out has no tap on any map


# ---- position, pixel, window ----------------------------------------------------------------------------------------------------------
def position(O, wcs, shape, sky):
    """Per point of sky (anything that reshapes to (N, 2) of (ra, dec)): (fin, x, y, i0, j0, fx, fy).  (x, y) is the oracle's
    batched sky2pix(safe=True), fin where both are finite; i0 = floor(x) under split_cell's clamp, fx = x - floor(x), exact in
    Float64, both 0 where the position is not finite.  Seven empty arrays for an empty batch."""
    nx, ny = int(shape[0]), int(shape[1])
    sky = np.ascontiguousarray(sky, dtype=np.float64).reshape(-1, 2)
    if sky.shape[0] == 0:
        z, zi = np.zeros(0), np.zeros(0, np.int64)
        return np.zeros(0, bool), z, z, zi, zi, z, z
    pix = O.sky2pix(wcs, (nx, ny), sky, safe=True)
    x, y = pix[:, 0], pix[:, 1]
    fin = np.isfinite(x) & np.isfinite(y)
    xs, ys = np.where(fin, x, 0.0), np.where(fin, y, 0.0)
    flx, fly = np.floor(xs), np.floor(ys)
    i0 = np.clip(flx, -CELL_LIMIT, CELL_LIMIT).astype(np.int64)
    j0 = np.clip(fly, -CELL_LIMIT, CELL_LIMIT).astype(np.int64)
    return fin, x, y, i0, j0, xs - flx, ys - fly


def flat_index(i, j, ok, shape, periodic):
    """1-based pixel (i, j) -> flat index into the full (ny, nx) plane, -1 for none: where ok is False, where the row is outside
    [1, ny], and where the column is outside [1, nx] unless the map is periodic, where it wraps."""
    nx, ny = int(shape[0]), int(shape[1])
    if periodic:
        i = (i - 1) % nx + 1
    else:
        ok = ok & (i >= 1) & (i <= nx)
    return np.where(ok & (j >= 1) & (j <= ny), (j - 1) * nx + (i - 1), -1)


def rows(shape, row0, nrows):
    """(row0, nrows) as ints, nrows None meaning every row from row0 to the map's last."""
    return int(row0), (int(shape[1]) - int(row0) if nrows is None else int(nrows))


def window(idx, shape, row0, nrows, rule, what="tap"):
    """Flat indices into the full (ny, nx) plane (-1: no tap) -> flat indices into the resident rows [row0, row0 + nrows).  A tap
    that is on the map but outside them is dropped (-1) under rule "drop", the device's rule, and raises under rule "raise":
    the banded yardsticks never drop one silently.  The whole map is its own window under either rule."""
    assert rule in ("drop", "raise"), rule
    nx = int(shape[0])
    row0, nrows = rows(shape, row0, nrows)
    idx = np.asarray(idx, dtype=np.int64)
    on = idx >= 0
    row = idx // nx
    out = on & ((row < row0) | (row >= row0 + nrows))
    if rule == "raise" and out.any():
        raise ValueError("%s: %d taps on rows %d .. %d, outside the resident rows [%d, %d)"
                         % (what, int(out.sum()), int(row[out].min()), int(row[out].max()), row0, row0 + nrows))
    return np.where(on & ~out, idx - row0 * nx, -1)


# ---- sums over the taps ---------------------------------------------------------------------------------------------------------------
def _taps2d(idx, w):
    idx = np.asarray(idx, dtype=np.int64)
    idx = idx[:, None] if idx.ndim == 1 else idx
    return idx, (np.ones(idx.shape) if w is None else np.asarray(w, dtype=np.float64).reshape(idx.shape))


def accumulate(idx, w, vals, size, out=None, bincount=False):
    """idx, w (N, T) (or (N,); w None: weight 1, and 1.0 * v is v to the bit); vals (nc, N) or (N,); out: the initial (nc, size)
    values or None (zeros, not counted as a term).  Returns (ref, k, S), each (nc, size): the np.add.at sum of the terms
    w[:, t] * vals[c] -- taps outer, planes inner, points in order --, their number and the sum of their magnitudes per slot, an
    initial `out` counted as one term.  bincount: the form S is summed in (the module docstring)."""
    idx, w = _taps2d(idx, w)
    vals = np.atleast_2d(np.asarray(vals, dtype=np.float64))
    nc = vals.shape[0]
    if out is None:
        ref = np.zeros((nc, size))
        k = np.zeros((nc, size), np.int64)
    else:
        ref = np.array(out, dtype=np.float64).reshape(nc, size).copy()
        k = np.ones((nc, size), np.int64)
    S = np.abs(ref)
    for t in range(idx.shape[1]):
        on = idx[:, t] >= 0
        at = idx[on, t]
        k += np.bincount(at, minlength=size)
        for c in range(nc):
            term = w[on, t] * vals[c, on]
            np.add.at(ref[c], at, term)
            if bincount:
                S[c] += np.bincount(at, weights=np.abs(term), minlength=size)
            else:
                np.add.at(S[c], at, np.abs(term))
    return ref, k, S


def nonzero_terms(idx, w, vals, size):
    """(nc, size): how many of a slot's terms w[:, t] * vals[c] are not zero (NaN counts), an initial map not counted.  With at
    most one the slot is added to once at most whatever the order, so the device must give the yardstick's bits there."""
    idx, w = _taps2d(idx, w)
    vals = np.atleast_2d(np.asarray(vals, dtype=np.float64))
    nz = np.zeros((vals.shape[0], size), np.int64)
    for t in range(idx.shape[1]):
        on = idx[:, t] >= 0
        for c in range(vals.shape[0]):
            term = w[on, t] * vals[c, on]
            nz[c] += np.bincount(idx[on, t][term != 0], minlength=size)
    return nz


def matrix(idx, w, size, resp=None, sparse=False):
    """The matrix of P from its taps, (N, size): row k holds w_t at column idx_t.  With resp the matrix of the polarised P,
    (N, 3 * size): r_c[k] * w_t at column c * size + idx_t, r = (1, q, u).  Taps of one point that meet on one pixel add up.
    Dense (np.add.at into zeros, so a -0.0 entry comes out +0.0) or a scipy.sparse CSR matrix."""
    idx, w = _taps2d(idx, w)
    n = len(idx)
    if resp is None:
        r = [np.ones(n)]
    else:
        resp = np.asarray(resp, dtype=np.float64).reshape(-1, 2)
        r = [np.ones(n), resp[:, 0], resp[:, 1]]
    rws, cols, vals = [], [], []
    for t in range(idx.shape[1]):
        on = np.flatnonzero(idx[:, t] >= 0)
        for c in range(len(r)):
            rws.append(on); cols.append(c * size + idx[on, t]); vals.append(r[c][on] * w[on, t])
    rws, cols, vals = np.concatenate(rws), np.concatenate(cols), np.concatenate(vals)
    if sparse:
        import scipy.sparse as sp
        return sp.csr_matrix((vals, (rws, cols)), shape=(n, len(r) * size))
    A = np.zeros((n, len(r) * size))
    np.add.at(A, (rws, cols), vals)
    return A


def adjoint_gap(m, pm, d, ref, S, roundings):
    """|<P m, d> - <m, P^T d>| and its bound 2^-53 * sum_p |m_p| * S_p * roundings_p, dot products in longdouble.  roundings is
    the per-pixel count each yardstick derives for its operator (8 + 2 k bilinear, 2 k nearest, 2 k + 2 nearest polarised)."""
    L = np.longdouble
    lhs = np.sum(np.asarray(pm).astype(L) * np.atleast_2d(d).astype(L))
    rhs = np.sum(m.reshape(ref.shape).astype(L) * ref.astype(L))
    b = 2.0 ** -53 * np.sum(np.abs(m.reshape(ref.shape)).astype(L) * S.astype(L) * roundings.astype(L))
    return float(abs(lhs - rhs)), float(b)


# ---- the named geometries of the yardsticks and the device tests ----------------------------------------------------------------------
def _box(nx, ny, cell):
    return lambda pj: pj.geometry([[nx * cell / 2 * DEG, -nx * cell / 2 * DEG], [-ny * cell / 2 * DEG, ny * cell / 2 * DEG]], cell * DEG)


def _fejer1(pj):
    _shape, w = pj.fullsky_geometry(1.0 * DEG)
    return (360, 180), pj.CarFejer1(w.cdelt, (w.crpix[0], 90.5), w.crval)          # rows at half-pixel offsets, one row fewer


GEOMETRIES = {                                  # name -> (builder, expected shape)
    "cc_360x181": (lambda pj: pj.fullsky_geometry(1.0 * DEG), (360, 181)),          # the 1 degree full sky (periodic)
    "cc_1024x513": (lambda pj: pj.fullsky_geometry(2 * np.pi / 1024), (1024, 513)),
    "cc_90x46": (lambda pj: pj.fullsky_geometry(4.0 * DEG), (90, 46)),
    "fejer1_360x180": (_fejer1, (360, 180)),
    "box_80x40": (_box(80, 40, 0.5), (80, 40)),                                     # the reference's 0.5 degree box
    "box_24x12": (_box(24, 12, 1.0), (24, 12)),
    "box_5x7": (_box(5, 7, 1.0), (5, 7)),
    "box_4x4": (_box(4, 4, 1.0), (4, 4)),                                           # every cubic tap row and column folds
    "box_2x2": (_box(2, 2, 1.0), (2, 2)),
    "box_1x1": (_box(1, 1, 1.0), (1, 1)),
}


def geometries(pj, names):
    """name -> (shape, wcs) for the names asked for, each built as the table says and checked against its expected shape."""
    g = {}
    for name in names:
        build, expect = GEOMETRIES[name]
        g[name] = build(pj)
        assert tuple(g[name][0][:2]) == expect, (name, g[name][0])
    return g
