"""numpy yardstick for the polarised pointing matrix, CPU only: P_pol (pj.sample_pol), P_pol^T
(pj.scatter_pol) and the weights mode (pj.scatter_pol_weights).

Nothing here is new arithmetic.  The forward composes the scalar samplers' yardsticks (the oracle's bilinear sampler; spline_ref's
prefilter and scattered evaluation) with

    out[k] = (s_I + q_k * s_Q) + u_k * s_U,

and the transposes hand the products

    t_0 = v, t_1 = q * v, t_2 = u * v, t_3 = q * t_1, t_4 = q * t_2, t_5 = u * t_2

to the scalar scatters' yardsticks (scatter_ref.scatter, scatter_cubic_ref.scatter and prefilter_transpose), one plane per
product.  Every product and sum is a separate numpy operation: one rounding each, nothing fuses.  The (ref, k, S) triples and
the bound k * 2^-52 * S per pixel are scatter_ref's.  tests/test_pol_ref.py holds this file to the dense matrix of P_pol and to
the adjoint identity."""
import numpy as np

import scatter_cubic_ref
import scatter_ref
import spline_ref
import tap_ref


def terms(v, resp, mode=0):
    """The values each plane receives: (3, N) for mode 0 (I, Q, U), (6, N) for mode 1 (II, IQ, IU, QQ, QU, UU)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    resp = np.asarray(resp, dtype=np.float64).reshape(-1, 2)
    q, u = resp[:, 0], resp[:, 1]
    t1 = q * v
    t2 = u * v
    t = [v, t1, t2]
    if mode:
        t += [q * t1, q * t2, u * t2]
    return np.stack(t)


def combine(s, resp):
    """(s_I + q s_Q) + u s_U from the (3, N) per-plane samples, left to right."""
    resp = np.asarray(resp, dtype=np.float64).reshape(-1, 2)
    a = resp[:, 0] * s[1]
    b = s[0] + a
    c = resp[:, 1] * s[2]
    return b + c


def sample_planes(O, wcs, shape, m, sky, order=1, prefiltered=False, row0=0, nrows=None):
    """The scalar samplers' yardstick, (nc, N): order 1 the oracle's bilinear sampler (m holds rows [row0, row0 + nrows));
    order 3 spline_ref's evaluation at the oracle's positions, of spline_ref's coefficients unless m already holds them (a band
    of rows only as coefficients; a tap outside it raises).  NaN where the position is not finite."""
    nx, ny = int(shape[0]), int(shape[1])
    m = np.asarray(m, dtype=np.float64)
    sky = np.ascontiguousarray(sky, dtype=np.float64).reshape(-1, 2)
    if order == 1:
        return O.sample_bilinear(wcs, (nx, ny, m.shape[0]), m, sky, row0, ny - row0 if nrows is None else nrows)
    per = bool(O.is_periodic(wcs, nx))
    fin, x, y = tap_ref.position(O, wcs, shape, sky)[:3]
    if len(fin) == 0:
        return np.zeros((m.shape[0], 0))
    x, y = np.where(fin, x, -10.0), np.where(fin, y, -10.0)
    if tap_ref.rows(shape, row0, nrows) != (0, ny):
        assert prefiltered, "a band of rows can only be given as coefficients"
        return np.where(fin[None, :], spline_ref.evaluate_points(m, x, y, per, row0=row0, ny=ny), np.nan)
    c = m if prefiltered else spline_ref.prefilter(m, per)
    return np.where(fin[None, :], spline_ref.evaluate_points(c, x, y, per), np.nan)


def sample(O, wcs, shape, m, sky, resp, order=1, prefiltered=False, row0=0, nrows=None):
    """P_pol m, (N,): m is the (3, nrows, nx) IQU map."""
    assert np.asarray(m).shape[0] == 3
    return combine(sample_planes(O, wcs, shape, m, sky, order, prefiltered, row0, nrows), resp)


def scatter(O, wcs, shape, sky, vals, resp, order=1, mode=0, out=None, row0=0, nrows=None):
    """The kernels' transpose (order 3: E^T alone).  vals (N,); out: initial (3 or 6, nrows, nx) map or None.
    Returns (ref, k, S) as tap_ref.accumulate forms them, one plane per product of terms()."""
    t = terms(vals, resp, mode)
    if order == 1:
        return scatter_ref.scatter(O, wcs, shape, sky, t, out=out, row0=row0, nrows=nrows)
    return scatter_cubic_ref.scatter(O, wcs, shape, sky, t, out=out, row0=row0, nrows=nrows)


def nonzero_terms(O, wcs, shape, sky, vals, resp, order=1, mode=0, row0=0, nrows=None):
    """(3 or 6, nrows, nx): how many of a pixel's terms are not zero (NaN counts), an initial map not counted
    (tap_ref.nonzero_terms of the order's taps)."""
    nx, nrows = int(shape[0]), tap_ref.rows(shape, row0, nrows)[1]
    idx, w = (scatter_ref.taps if order == 1 else scatter_cubic_ref.taps)(O, wcs, shape, sky, row0, nrows)
    nz = tap_ref.nonzero_terms(idx, w, terms(vals, resp, mode), nrows * nx)
    return nz.reshape(len(nz), nrows, nx)


def scatter_full(O, wcs, shape, sky, vals, resp, order=1, mode=0):
    """P_pol^T d into zeros: order 1 scatter(); order 3 F^T of it.  Returns (ptd, g, k, S), g the E^T map (ptd itself at order 1)."""
    g, k, S = scatter(O, wcs, shape, sky, vals, resp, order, mode)
    if order == 1:
        return g, g, k, S
    return scatter_cubic_ref.prefilter_transpose(g, bool(O.is_periodic(wcs, int(shape[0])))), g, k, S


def dense(O, wcs, shape, sky, resp, order=1):
    """The matrix of P_pol on coefficients (order 3: of E_pol, the prefilter left out), (N, 3 * ny * nx), straight from the taps:
    row k holds r_c[k] * w_t at column c * ny * nx + idx_t with r = (1, q, u).  Taps that fold onto one pixel add up."""
    idx, w = (scatter_ref.taps if order == 1 else scatter_cubic_ref.taps)(O, wcs, shape, sky)
    return tap_ref.matrix(idx, w, int(shape[0]) * int(shape[1]), resp)


def forward_rounding(s, resp, d):
    """2^-53 * 5 * sum_k |d_k| (|s_I| + |q s_Q| + |u s_U|): what the combination's own roundings may move <P_pol m, d> by.
    First order: one rounding on q s_Q, one on the first sum (|s_I| + |q s_Q|), one on u s_U, one on the last sum (all three),
    at most 3 on any summand; one more for the product q d or u d on the transpose's side; the fifth covers the second-order
    terms, which are 2^-53 of these."""
    resp = np.asarray(resp, dtype=np.float64).reshape(-1, 2)
    L = np.longdouble
    a = np.abs(s[0]).astype(L) + np.abs(resp[:, 0] * s[1]).astype(L) + np.abs(resp[:, 1] * s[2]).astype(L)
    return float(2.0 ** -53 * 5 * np.sum(np.abs(np.asarray(d)).astype(L) * a))
