"""numpy yardstick of the banded-Toeplitz noise weight, CPU only: pxl_tod_toeplitz_f64 / pj.toeplitz_tod and the
dense form of the map pj.ml_map_pol_nearest_tod solves for.

THE DEFINITION (include/pixell_hip.h).  Segment s is [seg[s], seg[s+1]) with both ends clamped to [0, T] (fit_ref.clamp).  A sample
is LIVE when it lies in a segment and wlive > 0 (NaN is not; None: every sample).  z = x at the live samples and +0.0 elsewhere,
and +0.0 outside the segment of the output at hand.  For a live sample t

    S = c_0 * z_t;    S = S + c_k * (z_(t-k) + z_(t+k))  for k = 1 .. lambda in that order;    out_t = S

and every other sample is +0.0.  apply() evaluates exactly that, vectorised over t, so numpy performs the operations of the
definition one by one in its order: in Float64 its result is the device's bit for bit.  With dtype=np.longdouble it is the
reference of the accuracy bound: a term c_k * (zl + zr) carries two roundings and the lambda adds one each, so the Float64 form is
within (lambda + 2) 2^-53 Sabs of the exact sum, Sabs = |c_0| |z_t| + sum_k |c_k| (|z_(t-k)| + |z_(t+k)|) -- bound() returns
(lambda + 3) 2^-52 Sabs, the issue's figure, more than twice that."""
import numpy as np

import fit_ref
import nearest_ref
import polsolve_ref

EPS = 2.0 ** -52
TILE = 1280                                                     # the device's tile, PXL_TOEP_C of csrc/pxl_toeplitz.h
LAMBDA_MAX = 4096


def live_mask(shape, seg, wlive):
    """(D, T) bool: in a (clamped) segment and wlive > 0."""
    nd, nt = shape
    inside = np.zeros(nt, dtype=bool)
    for lo, hi in fit_ref.clamp(seg, nt):
        inside[lo:hi] = True
    live = np.broadcast_to(inside, (nd, nt)).copy()
    if wlive is not None:
        with np.errstate(invalid="ignore"):
            live &= np.asarray(wlive, dtype=np.float64) > 0
    return live


def _taps(x, kern, seg, wlive, dtype, absolute):
    x = np.asarray(x, dtype=np.float64)
    nd, nt = x.shape
    c = np.broadcast_to(np.asarray(kern, dtype=np.float64), (nd, np.shape(kern)[-1])).astype(dtype)
    lam = c.shape[1] - 1
    live = live_mask(x.shape, seg, wlive)
    out = np.zeros((nd, nt), dtype=dtype)
    if absolute:
        c = np.abs(c)
    with np.errstate(all="ignore"):
        for lo, hi in fit_ref.clamp(seg, nt):                   # in the order of s: where segments overlap the later one stands
            L = hi - lo
            if L == 0:
                continue
            z = np.zeros((nd, L + 2 * lam), dtype=dtype)
            zin = np.where(live[:, lo:hi], x[:, lo:hi], 0.0).astype(dtype)      # an x under a cut enters no arithmetic
            z[:, lam:lam + L] = np.abs(zin) if absolute else zin
            S = c[:, 0:1] * z[:, lam:lam + L]
            for k in range(1, lam + 1):
                S = S + c[:, k:k + 1] * (z[:, lam - k:lam - k + L] + z[:, lam + k:lam + k + L])
            out[:, lo:hi] = np.where(live[:, lo:hi], S, dtype(0.0))
    return out


def apply(x, kern, seg, wlive=None, dtype=np.float64):
    """out (D, T) of the definition in `dtype`.  x (D, T); kern (D, lambda + 1) or (lambda + 1,); seg the n_seg + 1 offsets, any
    contents; wlive (D, T) or None."""
    return _taps(x, kern, seg, wlive, dtype, False)


def bound(x, kern, seg, wlive=None):
    """(lambda + 3) 2^-52 Sabs per sample, (D, T) Float64 (the module's docstring); inf or NaN where Sabs is."""
    lam = np.shape(kern)[-1] - 1
    return (lam + 3) * EPS * _taps(x, kern, seg, wlive, np.float64, True)


def dense_gtg(kern_row, seg, live_row):
    """The (T, T) matrix G T G of one detector: T[i, j] = c_|i-j| where |i - j| <= lambda and i, j lie in one segment, G the
    diagonal of live_row.  For tiny cases."""
    c = np.asarray(kern_row, dtype=np.float64)
    lam, nt = len(c) - 1, len(live_row)
    sid = np.full(nt, -1)
    for s, (lo, hi) in enumerate(fit_ref.clamp(seg, nt)):
        sid[lo:hi] = s
    i = np.arange(nt)
    dist = np.abs(i[:, None] - i[None, :])
    T = np.where((dist <= lam) & (sid[:, None] == sid[None, :]) & (sid[:, None] >= 0), c[np.minimum(dist, lam)], 0.0)
    g = np.asarray(live_row, dtype=np.float64)
    return g[:, None] * T * g[None, :]


class MLSystem:
    """The dense form of pj.ml_map_pol_nearest_tod on nearest_ref's pixels, everything that does not depend on the timestream.
    sky, resp (D * T, 2) detector-major; w (D, T), which only flags; kern (D, lambda + 1).  Holds: the white-noise planes w6
    (6, ny, nx) and rcond (ny, nx) of the weights c_0 [w > 0], solved (ny, nx) = rcond >= rcond_min, g (D, T) = [w > 0] and on a
    solved pixel, A = P^T G T G P on the solved pixels (columns plane-major: plane * n_solved + pixel), cond (of A) and pcond (of
    M^-1/2 A M^-1/2, M the pixel blocks of w6)."""

    def __init__(self, O, wcs, shape, sky, resp, kern, seg, w, rcond_min):
        w, kern = np.asarray(w, dtype=np.float64), np.asarray(kern, dtype=np.float64)
        self.args = (O, wcs, shape, sky, resp)
        self.nd, self.nt = nd, nt = w.shape
        self.nx, self.ny = nx, ny = int(shape[0]), int(shape[1])
        self.rcond_min = rcond_min
        self.flag = w > 0
        self.w1 = (kern[:, 0:1] * self.flag).reshape(-1)
        (_rhs, _k, _S), (w6, _k6, _S6) = nearest_ref.bin(O, wcs, shape, sky, resp, np.zeros(nd * nt), self.w1)
        _x, rc, _info = polsolve_ref.solve(w6.reshape(6, -1), np.zeros((3, nx * ny)), rcond_min)
        self.w6, self.rcond = w6, rc.reshape(ny, nx)
        solved = rc >= rcond_min
        self.solved = solved.reshape(ny, nx)
        idx = nearest_ref.taps(O, wcs, shape, sky)[0].reshape(nd, nt)
        self.g = self.flag & (idx >= 0) & solved[np.maximum(idx, 0)]
        self.cols = np.concatenate([p * nx * ny + np.flatnonzero(solved) for p in range(3)])
        P = nearest_ref.dense(O, wcs, shape, sky, resp)[:, self.cols].reshape(nd, nt, len(self.cols))
        A = np.zeros((len(self.cols), len(self.cols)))
        self.NP = []
        for det in range(nd):
            NP = dense_gtg(kern[det], seg, self.g[det]) @ P[det]
            A += P[det].T @ NP
            self.NP.append(NP)
        self.A = 0.5 * (A + A.T)
        ns = int(solved.sum())
        M = np.zeros_like(A)
        blocks = polsolve_ref.dense(w6.reshape(6, -1)[:, solved])                # (ns, 3, 3)
        for p in range(3):
            for q in range(3):
                M[p * ns + np.arange(ns), q * ns + np.arange(ns)] = blocks[:, p, q]
        Li = np.linalg.inv(np.linalg.cholesky(M))
        ev = np.linalg.eigvalsh(Li @ self.A @ Li.T)
        self.cond, self.pcond = float(np.linalg.cond(self.A)), float(ev[-1] / ev[0])

    def solve(self, tod):
        """The ML map (3, ny, nx) of the (D, T) timestream, +0.0 on the unsolved pixels; a value under a cut is not read."""
        b = sum(NP.T @ np.where(g, d, 0.0) for NP, g, d in zip(self.NP, self.g, np.asarray(tod, dtype=np.float64)))
        m = np.zeros(3 * self.nx * self.ny)
        m[self.cols] = np.linalg.solve(self.A, b)
        return m.reshape(3, self.ny, self.nx)

    def binned(self, tod):
        """The white-noise binned map of the same timestream with the weights c_0 [w > 0]."""
        O, wcs, shape, sky, resp = self.args
        d0 = np.where(self.flag, np.asarray(tod, dtype=np.float64), 0.0).reshape(-1)
        (rhs, _k, _S), _w = nearest_ref.bin(O, wcs, shape, sky, resp, d0, self.w1)
        x, _rc, _info = polsolve_ref.solve(self.w6.reshape(6, -1), rhs.reshape(3, -1), self.rcond_min)
        return x.reshape(3, self.ny, self.nx)
