"""The per-scan polynomial filter in numpy, twice: in Float64 with every sum sequential in index order, and in
np.longdouble.  Both follow include/pixell_hip.h's definition operation for operation (numpy never fuses a product into a
sum); the device differs from the Float64 form only in the order of the moment sums (lanes stride, a tree joins them).  That
order is held here too: lanes=G gives the Float64 form with the sums of a group of G lanes, which the device must match to the bit.

filter(d, seg_start, order, wfit=None, rcond_min=1e-10, dtype=np.float64, lanes=None) -> Fit(out, coeffs, n_used, ratios): out (D, T),
coeffs (D, S, order + 1), n_used (D, S) and ratios (D, S, order + 1), the pivot ratio D_i / G_ii of every pivot that was formed
(NaN for the pivots past the first rejected one, which the definition never forms, and for an empty segment)."""
import collections

import numpy as np

import fit_ref

Fit = collections.namedtuple("Fit", "out coeffs n_used ratios")


def group(n_t, n_seg, order):
    """The number of lanes G that own one (detector, segment): the host's rule, from n_t, n_seg and the order alone."""
    mean = n_t // max(n_seg, 1)
    if mean >= 1024:
        return 256
    lanes = (mean + order) // (order + 1)
    g = 1
    while g < 64 and g < lanes:
        g *= 2
    return g


clamp_segments = fit_ref.clamp          # the segments along the n_t samples of a detector


def legendre(x, order, ft):
    """P_0 .. P_order at the array x, in the definition's order of operations."""
    P = [np.ones_like(x)]
    if order >= 1:
        P.append(x.copy())
    for n in range(1, order):
        P.append(((ft(2 * n + 1) * x) * P[n] - ft(n) * P[n - 1]) / ft(n + 1))
    return P


def basis(L, order, ft=np.float64):
    j = np.arange(L, dtype=np.int64)
    x = ((2 * j + 1) - L).astype(ft) / ft(L)
    return legendre(x, order, ft)


def _seq_sum(terms, ft):
    s = ft(0.0)
    for t in terms:
        s = s + t
    return s


_tree = fit_ref.tree


def _lane_sum(terms, live, lanes):
    """The device's order: lane l adds the live terms l, l + lanes, ... in order from +0.0 (a term that is not live is replaced by
    +0.0, which changes no bit of a sum that starts at +0.0), then the fixed tree; 256 lanes are four wavefronts, (s0 + s1) + (s2 + s3)."""
    rows = -(-len(terms) // lanes)
    t = np.zeros(rows * lanes)
    t[:len(terms)] = np.where(live, terms, 0.0)
    acc = np.zeros(lanes)
    for row in t.reshape(rows, lanes):
        acc = acc + row
    if lanes == 256:
        s = [_tree(acc[k * 64:(k + 1) * 64]) for k in range(4)]
        return (s[0] + s[1]) + (s[2] + s[3])
    return _tree(acc)


def solve(G, b, rcond_min, ft):
    """LDL^T without pivoting, truncated at the first rejected pivot: (c, n_used, ratios).  G is the full symmetric matrix."""
    n = len(b)
    Lm = np.zeros((n, n), dtype=ft)
    D = np.zeros(n, dtype=ft)
    ratios = np.full(n, np.nan, dtype=ft)
    nu = 0
    for i in range(n):
        u = np.zeros(n, dtype=ft)
        dd = G[i, i]
        for k in range(i):
            s = G[i, k]
            for m in range(k):
                s = s - u[m] * Lm[k, m]
            u[k] = s
            Lm[i, k] = s / D[k]
            dd = dd - s * Lm[i, k]
        D[i] = dd
        with np.errstate(all="ignore"):
            ratios[i] = dd / G[i, i]
            ok = dd > ft(rcond_min) * G[i, i]
        if not ok:
            break
        nu = i + 1
    y = np.zeros(n, dtype=ft)
    c = np.zeros(n, dtype=ft)
    for i in range(nu):
        s = b[i]
        for m in range(i):
            s = s - Lm[i, m] * y[m]
        y[i] = s
    for i in range(nu - 1, -1, -1):
        s = y[i] / D[i]
        for m in range(i + 1, nu):
            s = s - Lm[m, i] * c[m]
        c[i] = s
    return c, nu, ratios


def filter(d, seg_start, order, wfit=None, rcond_min=1e-10, dtype=np.float64, lanes=None):
    ft = dtype
    assert lanes is None or dtype is np.float64
    d = np.asarray(d, dtype=np.float64)
    nd, nt = d.shape
    segs = clamp_segments(seg_start, nt)
    out = d.astype(ft)
    npoly = order + 1
    coeffs = np.zeros((nd, len(segs), npoly), dtype=ft)
    n_used = np.zeros((nd, len(segs)), dtype=np.int64)
    ratios = np.full((nd, len(segs), npoly), np.nan, dtype=ft)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, (lo, hi) in enumerate(segs):
            L = hi - lo
            if L == 0:
                continue
            P = basis(L, order, ft)
            for det in range(nd):
                w = np.ones(L, dtype=ft) if wfit is None else np.asarray(wfit[det, lo:hi]).astype(ft)
                live = np.flatnonzero(w > 0)
                dv = d[det, lo:hi].astype(ft)
                G = np.zeros((npoly, npoly), dtype=ft)
                b = np.zeros(npoly, dtype=ft)
                for i in range(npoly):
                    if lanes is None:
                        wp = w[live] * P[i][live]
                        for k in range(i + 1):
                            G[i, k] = G[k, i] = _seq_sum(wp * P[k][live], ft)
                        b[i] = _seq_sum(wp * dv[live], ft)
                    else:
                        wp = w * P[i]
                        for k in range(i + 1):
                            G[i, k] = G[k, i] = _lane_sum(wp * P[k], w > 0, lanes)
                        b[i] = _lane_sum(wp * dv, w > 0, lanes)
                c, nu, r = solve(G, b, rcond_min, ft)
                coeffs[det, s], n_used[det, s], ratios[det, s] = c, nu, r
                if nu == 0:
                    continue
                f = np.full(L, c[0], dtype=ft)
                for n in range(1, npoly):
                    f = f + c[n] * P[n]
                out[det, lo:hi] = dv - f
    return Fit(out, coeffs, n_used, ratios)


def projector(L, order, wfit):
    """fit_ref.projector of one full-rank segment of L samples."""
    return fit_ref.projector(np.stack(basis(L, order, np.longdouble), axis=1), wfit)
