"""numpy yardstick for nearest-pixel (order 0) pointing, CPU only: pj.sample_nearest, pj.scatter_nearest, their
polarised forms, pj.bin_pol_nearest and the map pj.binned_map_pol_nearest makes of them.

Definition: for point k, (x, y) is the oracle's batched sky2pix(safe=True) in the reciprocal form, the position of the order-1
yardstick (both are tap_ref.position) and, bit for bit, the device's.  With i0 = floor(x), fx = x - i0 (exact in Float64), the pixel is

    i = i0 + (fx >= 0.5),   j = j0 + (fy >= 0.5):

pixel i owns [i - 0.5, i + 0.5), a tie goes to the higher index, and the rule has no rounding of its own.  i0 and j0 carry
split_cell's clamp.  Columns wrap on a full-circle map and are off the map outside [1, nx] otherwise; rows are on the map inside
[1, ny] and inside the window.  A sample is the pixel's value unchanged, +0.0 off the map, NaN where the position is not finite; a
scatter adds the value itself to that pixel.  The polarised forms hand pol_ref.terms / pol_ref.combine's products to them.

What differs between this file and the device is the ORDER of the additions into one pixel, so the transposes are held to
scatter_ref's bound k * 2^-52 * S per pixel through the same (ref, k, S) triples.  tests/test_nearest_ref.py holds this file to
its dense matrix, to the adjoint identity, to scatter_ref's taps and to scipy.ndimage.map_coordinates(order=0)."""
import numpy as np

import pol_ref
import polsolve_ref
import scatter_ref
import tap_ref

EPS = 2.0 ** -52


def cells(O, wcs, shape, sky, row0=0, nrows=None):
    """Everything the rule forms per point: (idx, fin, i, j, fx, fy).  idx is the flat index into the resident (nrows, nx) plane,
    -1 off the map or where the position is not finite; i, j the 1-based pixel before wrapping; fx, fy the exact fractions
    (0 where the position is not finite)."""
    fin, _x, _y, i0, j0, fx, fy = tap_ref.position(O, wcs, shape, sky)
    i, j = i0 + (fx >= 0.5), j0 + (fy >= 0.5)
    idx = tap_ref.flat_index(i, j, fin, shape, O.is_periodic(wcs, int(shape[0])))
    return tap_ref.window(idx, shape, row0, nrows, "drop"), fin, i, j, fx, fy


def taps(O, wcs, shape, sky, row0=0, nrows=None):
    """(idx (N,), ): per point the flat index of its pixel in the resident (nrows, nx) plane, -1 for a point that has none."""
    return (cells(O, wcs, shape, sky, row0, nrows)[0],)


def classes(O, wcs, shape, sky):
    """Per axis, where the fraction lies: (cx, cy), each (N,) of 0 (== 0.5, the tie), -1 (below) or +1 (above); 2 where the
    position is not finite."""
    _idx, fin, _i, _j, fx, fy = cells(O, wcs, shape, sky)
    return tuple(np.where(fin, np.sign(f - 0.5).astype(np.int64), 2) for f in (fx, fy))


def sample(O, wcs, shape, m, sky, row0=0, nrows=None):
    """P m per plane, (nc, N): m holds rows [row0, row0 + nrows) of every plane.  The pixel's value as bits, +0.0 off the map,
    NaN where the position is not finite."""
    m = np.asarray(m, dtype=np.float64)
    m = m.reshape((-1,) + m.shape[-2:])
    idx, fin = cells(O, wcs, shape, sky, row0, nrows)[:2]
    flat = m.reshape(m.shape[0], -1)
    out = np.zeros((m.shape[0], len(idx)))
    on = idx >= 0
    out[:, on] = flat[:, idx[on]]
    out[:, ~fin] = np.nan
    return out


def scatter(O, wcs, shape, sky, vals, out=None, row0=0, nrows=None):
    """vals (nc, N) or (N,); out: initial (nc, nrows, nx) map or None (zeros, not counted as a term).  Returns (ref, k, S) as
    scatter_ref.scatter does: tap_ref.accumulate with one tap of weight 1."""
    nx, nrows = int(shape[0]), tap_ref.rows(shape, row0, nrows)[1]
    idx = taps(O, wcs, shape, sky, row0, nrows)[0]
    return tuple(a.reshape(len(a), nrows, nx) for a in tap_ref.accumulate(idx, None, vals, nrows * nx, out))


def nonzero_terms(O, wcs, shape, sky, vals, row0=0, nrows=None):
    """(nc, nrows, nx): tap_ref.nonzero_terms of the one tap."""
    nx, nrows = int(shape[0]), tap_ref.rows(shape, row0, nrows)[1]
    nz = tap_ref.nonzero_terms(taps(O, wcs, shape, sky, row0, nrows)[0], None, vals, nrows * nx)
    return nz.reshape(len(nz), nrows, nx)


def sample_pol(O, wcs, shape, m, sky, resp, row0=0, nrows=None):
    """(s_I + q s_Q) + u s_U of sample()'s per-plane values, (N,)."""
    assert np.asarray(m).shape[0] == 3
    with np.errstate(invalid="ignore", over="ignore"):
        return pol_ref.combine(sample(O, wcs, shape, m, sky, row0, nrows), resp)


def scatter_pol(O, wcs, shape, sky, vals, resp, mode=0, out=None, row0=0, nrows=None):
    """vals (N,); one plane per product of pol_ref.terms: 3 (mode 0) or 6 (mode 1).  Returns (ref, k, S)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return scatter(O, wcs, shape, sky, pol_ref.terms(vals, resp, mode), out=out, row0=row0, nrows=nrows)


def nonzero_terms_pol(O, wcs, shape, sky, vals, resp, mode=0, row0=0, nrows=None):
    with np.errstate(invalid="ignore", over="ignore"):
        return nonzero_terms(O, wcs, shape, sky, pol_ref.terms(vals, resp, mode), row0, nrows)


def bin(O, wcs, shape, sky, resp, d, w, rhs=None, weights=None, row0=0, nrows=None):
    """The fused pass as the composition its contract names: scatter_pol of w * d (one rounding) into rhs, scatter_pol in the
    weights mode of w into weights.  Returns two triples, ((ref, k, S) of rhs, (ref, k, S) of weights).  With row0, nrows: rhs,
    weights and the results hold rows [row0, row0 + nrows) of the full map; a pixel on the map outside them raises."""
    if tap_ref.rows(shape, row0, nrows) != (0, int(shape[1])):          # cells() DROPS a pixel outside the window: the device's rule
        tap_ref.window(taps(O, wcs, shape, sky)[0], shape, row0, nrows, "raise", "nearest pixel")
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(w, dtype=np.float64) * np.asarray(d, dtype=np.float64)
    return (scatter_pol(O, wcs, shape, sky, v, resp, 0, out=rhs, row0=row0, nrows=nrows),
            scatter_pol(O, wcs, shape, sky, w, resp, 1, out=weights, row0=row0, nrows=nrows))


def dense(O, wcs, shape, sky, resp=None):
    """The matrix of P, (N, ny * nx): row k is one-hot at its pixel (zero for a point that has none).  With resp the matrix of the
    polarised P, (N, 3 * ny * nx): r_c[k] at column c * ny * nx + idx, r = (1, q, u)."""
    return tap_ref.matrix(taps(O, wcs, shape, sky)[0], None, int(shape[0]) * int(shape[1]), resp)


def adjoint_gap(m, pm, d, ref, k, S):
    """|<P m, d> - <m, P^T d>| and its bound 2^-53 * sum_p |m_p| * S_p * 2 k_p for the scalar form, dot products in longdouble.
    P m is a copy and a term of P^T d is the value itself: no rounding on either side but the k_p adds of a pixel, in the
    yardstick's order (k_p * 2^-53 * S_p), and 2 k_p leaves as much for the device's order."""
    return tap_ref.adjoint_gap(m, pm, d, ref, S, 2 * k)


def adjoint_gap_pol(m, pm, d, ref, k, S, s, resp):
    """The polarised form: the transpose's terms carry one rounding (q d, u d), the 2 k_p of the adds becomes 2 k_p + 2, and the
    forward combination adds pol_ref.forward_rounding."""
    gap, b = tap_ref.adjoint_gap(m, pm, d, ref, S, 2 * k + 2)
    return gap, b + pol_ref.forward_rounding(s, resp, d)


# ---- the geometries and points of the device tests ------------------------------------------------------------------------------------
GEOMS = ("cc_360x181", "box_80x40", "box_5x7", "box_2x2", "box_1x1")


def geometries(pj):
    """name -> (shape, wcs): the 1 degree full sky (periodic), the reference's 0.5 degree box, and boxes of 5 x 7, 2 x 2 and 1 x 1."""
    return tap_ref.geometries(pj, GEOMS)


def edge_points(O, wcs, shape, shift=0.0, cap=None, seed=0):
    """The positions x = i + 0.5 + shift, y = j + 0.5 + shift for every i in [-1, nx + 1], j in [-1, ny + 1], as (ra, dec) from
    O.pix2sky: every pixel edge, the seam, the pole rows and one pixel beyond.  shift is in pixels, applied in pixel space
    (nudging the sky coordinate by a few ulps does not move a box point off the tie).  cap: keep at most that many, drawn without
    replacement, always with the four corners of the lattice."""
    nx, ny = shape
    xi, yj = np.arange(-1, nx + 2) + 0.5 + shift, np.arange(-1, ny + 2) + 0.5 + shift
    pix = np.stack(np.meshgrid(xi, yj, indexing="xy"), axis=-1).reshape(-1, 2)
    if cap is not None and len(pix) > cap:
        keep = np.random.default_rng(seed).choice(len(pix), cap, replace=False)
        keep[:4] = [0, len(xi) - 1, len(pix) - len(xi), len(pix) - 1]
        pix = pix[np.unique(keep)]
    return O.pix2sky(wcs, pix, O.WRAP_NONE)


NUDGE = 2.0 ** -30                 # pixels: far above the evaluators' rounding (1e-13 pixel), far below anything else


def points(O, wcs, shape, n, seed):
    """n points for the forward and transpose checks: over the map widened by 1.5 pixels, half of them uniform on the sphere on a
    full-sky map; then pixel-edge points (ties) as they are and nudged either way, pixel centres, points far outside; the last
    three positions are not finite."""
    nx, ny = shape
    rng = np.random.default_rng(seed)
    if O.is_periodic(wcs, nx):
        sky = np.concatenate([scatter_ref.sphere_points(n // 2, seed), scatter_ref.box_points(O, wcs, shape, n - n // 2, seed + 1)])
    else:
        sky = scatter_ref.box_points(O, wcs, shape, n, seed + 1)
    m = min(n // 8, 400)
    if m:
        special = [edge_points(O, wcs, shape, s, cap=m, seed=seed + 2 + t) for t, s in enumerate((0.0, -NUDGE, NUDGE))]
        centres = np.stack([rng.integers(1, nx + 1, m), rng.integers(1, ny + 1, m)], axis=1).astype(float)
        far = np.stack([rng.uniform(-3 * nx, 4 * nx, m), rng.uniform(-2.0 * ny, -1.0, m)], axis=1)
        special.append(O.pix2sky(wcs, np.concatenate([centres, far]), O.WRAP_NONE))
        special = np.concatenate(special)[:n]
        sky[:len(special)] = special
    if n >= 3:
        sky[-3:] = [[np.nan, 0.1], [0.2, np.inf], [-np.inf, np.nan]]
    return sky


def special_map(shape, nc, seed):
    """A map of N(0, 1) with NaN, +-Inf, -0.0, huge and subnormal pixels sown in (as many as fit)."""
    nx, ny = shape
    rng = np.random.default_rng(seed)
    m = rng.normal(size=(nc, ny, nx))
    flat = m.reshape(-1)
    vals = [np.nan, np.inf, -np.inf, -0.0, 1.7e308, -1.7e308, 5e-324, -2.5e-310, 0.0]
    at = rng.choice(flat.size, min(flat.size, 4 * len(vals)), replace=False)
    for t, p in enumerate(at[:max(1, flat.size - 1)]):                 # leave one ordinary pixel where there is room for one
        flat[p] = vals[t % len(vals)]
    return m


# ---- the map: noiseless samples of a random sky (test 8) -------------------------------------------------------------------------------
MAP_POINTS = {"box_5x7": 2 * 10 ** 4, "box_80x40": 2 * 10 ** 5, "cc_360x181": 50 * 360 * 181}      # at least 48 per pixel on average
RCOND_MIN = 1e-3
K0 = 50.0


class MapCase:
    """normal_ref.Case's inputs for the order-0 pointing matrix: n points uniform in pixel space, random psi, w = 10^U(-1, 1), a
    random sky m0 and its noiseless samples d = P m0 (this file's sample_pol: the device's forward bits), in three batches.  The
    points of three pixels are taken out, so the map has pixels without a hit."""

    def __init__(self, pj, O, geom, seed):
        import normal_ref
        self.geom = geom
        self.shape, self.wcs = geometries(pj)[geom]
        nx, ny = self.shape
        n = MAP_POINTS[geom]
        rng = np.random.default_rng(seed)
        sky = normal_ref.pixel_uniform(O, self.wcs, self.shape, n, rng)
        idx = taps(O, self.wcs, self.shape, sky)[0]
        self.unhit = np.array([3, (nx * ny) // 2, nx * ny - 1])         # three pixels whose points are taken out: no hits there
        self.sky = sky[~np.isin(idx, self.unhit)]
        n = len(self.sky)
        psi = rng.uniform(0, np.pi, n)
        self.resp = np.stack([np.cos(2 * psi), np.sin(2 * psi)], axis=1)
        self.w = 10.0 ** rng.uniform(-1, 1, n)
        self.m0 = rng.normal(size=(3, ny, nx))
        self.d = sample_pol(O, self.wcs, self.shape, self.m0, self.sky, self.resp)
        cut = (0, n // 3, n // 2, n)                                    # three batches of unequal length
        self.batches = [slice(cut[b], cut[b + 1]) for b in range(3)]
        (self.rhs, self.k, _S), (self.w6, _k6, _S6) = bin(O, self.wcs, self.shape, self.sky, self.resp, self.d, self.w)
        self.hits = self.k[0]                                           # (ny, nx): the pixel's term count
        x, rc, info = polsolve_ref.solve(self.w6.reshape(6, -1), self.rhs.reshape(3, -1), RCOND_MIN)
        self.map, self.rcond, self.solved = x.reshape(3, ny, nx), rc.reshape(ny, nx), info["ok"].reshape(ny, nx)
        with np.errstate(invalid="ignore", over="ignore"):
            self.nz_w = nonzero_terms_pol(O, self.wcs, self.shape, self.sky, self.w, self.resp, 1)


_map_cases = {}


def map_case(pj, O, geom):
    """The shared, unchanged inputs of the CPU and GPU map tests."""
    if geom not in _map_cases:
        _map_cases[geom] = MapCase(pj, O, geom, 90 + len(geom))
    return _map_cases[geom]


def map_bound(m0, hits, rcond):
    """16 (k + 50) 2^-52 ||m0(p)||_1 / rc(p) per pixel, (ny, nx): tests/test_gpu_polsolve.py::test_constant_sky_full_sky's
    derivation with the interpolation weight om = 1 (exact, as it is taken there) and the pixel's own sky triple in the place of
    the constant one -- with one pixel per point every sample of pixel p is (I0(p) + q Q0(p)) + u U0(p) and A(p) m0(p) = r(p) in
    exact arithmetic, which is all the derivation uses.  k is the pixel's term count, rc its rcond.  inf where rc is 0."""
    with np.errstate(divide="ignore"):
        return 16.0 * (hits + K0) * EPS * np.abs(m0).sum(axis=0) / rcond


# ---- P^T W P is the blocks (test 9) ----------------------------------------------------------------------------------------------------
def blocks_bound(O, wcs, shape, x, sky, resp, w):
    """Per plane and pixel, (3, ny, nx): what scatter_pol(w * sample_pol(x)) and polsolve_ref.apply(weights, x) may differ by,
    whichever order either side's adds arrive in.  Derived, nothing measured (u = 2^-53, k the pixel's term count, r = (1, q, u)):

      composition  d = (x0 + q x1) + u x2 is within 3u D of exact, D = |x0| + |q x1| + |u x2| (pol_ref.forward_rounding's count);
                   v = w d and t_c = r_c v add one rounding each: 5u w |r_c| D per term; the k adds, in any order, k u sum|term|.
                   Row c is within (5 + k) u Sabs_c of sum_k w r_c (r . x), Sabs_c = sum_k w |r_c| D_k.
      blocks       a weight term w r_c r_j carries at most 2 roundings and the k adds k u: plane cj is within (2 + k) u Wabs_cj,
                   Wabs_cj = sum_k w |r_c| |r_j|; the row (W_c0 x0 + W_c1 x1) + W_c2 x2 puts at most 3 more on each summand:
                   (5 + k) u sum_j Wabs_cj |x_j| = (5 + k) u Sabs_c.

    Together (10 + 2 k) u Sabs_c = (k + 5) 2^-52 Sabs_c; (k + 6) leaves one unit for the second-order terms and for Sabs itself,
    which is formed here in Float64 as the yardstick on |x|, |resp|, |w| (the S plane of that scatter: no cancellation)."""
    ax, ar, aw = np.abs(x), np.abs(resp), np.abs(w)
    v = aw * sample_pol(O, wcs, shape, ax, sky, ar)
    _ref, k, Sabs = scatter_pol(O, wcs, shape, sky, v, ar)
    return (k + 6.0) * EPS * Sabs
