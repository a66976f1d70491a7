"""The detector-mode filter in numpy, three times: in Float64 with every sum sequential in detector order, in
np.longdouble, and in Float64 in the device's order -- R = 256 / C row phases that stride the group's detectors, joined by the
tree v_p = v_p + v_(p ^ off), off = R/2 .. 1 -- with the host's rule for C (tile below).  All follow include/pixell_hip.h's
definition operation for operation (numpy never fuses a product into a sum); every array operation here runs over the time
samples, which are independent.  The solve is polyfilter_ref.solve's, written over a vector of columns (tests/test_modefilter_ref.py
holds the two to the same bits).

filter(d, modes, grp_start=None, wfit=None, rcond_min=1e-10, dtype=np.float64, phases=None) -> Fit(out, amps, n_used, ratios):
out (D, T), amps (n_grp, K, T), n_used (n_grp, T) and ratios (n_grp, K, T), the pivot ratio D_i / G_ii of every pivot that was
formed (NaN for the pivots past the first rejected one, which the definition never forms).  phases=R gives the device's order."""
import collections

import numpy as np

import fit_ref

Fit = collections.namedtuple("Fit", "out amps n_used ratios")


def tile(n_t, n_grp):
    """The number of time samples C a block owns: the host's rule, from n_t and n_grp alone.  R = 256 // C row phases."""
    return 64 if n_grp * ((n_t + 63) // 64) >= 512 else 16


clamp_groups = fit_ref.clamp            # the groups along the n_det detectors


def _sum(terms, live, ft, phases):
    """terms, live: (n, T).  Sequential from +0.0 over the live rows, or by phases: phase p takes rows p, p + R, ... in order, and
    the tree joins the phases.  A row that is not live adds nothing (its term, NaN or not, is never added)."""
    n, nt = terms.shape
    if phases is None:
        acc = np.zeros(nt, dtype=ft)
        for r in range(n):
            acc = np.where(live[r], acc + terms[r], acc)
        return acc
    acc = np.zeros((phases, nt), dtype=ft)
    for r in range(n):
        p = r % phases
        acc[p] = np.where(live[r], acc[p] + terms[r], acc[p])
    return fit_ref.tree(acc)


def solve(G, b, rcond_min, ft):
    """polyfilter_ref.solve over a vector of systems: G (K, K, T) symmetric, b (K, T) -> (c (K, T), n_used (T,), ratios (K, T)).
    LDL^T without pivoting, truncated per column at the first rejected pivot."""
    K, nt = b.shape
    Lm = np.zeros((K, K, nt), dtype=ft)
    D = np.zeros((K, nt), dtype=ft)
    ratios = np.full((K, nt), np.nan, dtype=ft)
    nu = np.zeros(nt, dtype=np.int64)
    alive = np.ones(nt, dtype=bool)
    err = np.seterr(all="ignore")                               # the columns past their truncation hold values nobody reads
    for i in range(K):
        u = np.zeros((K, nt), dtype=ft)
        dd = G[i, i].copy()
        for k in range(i):
            s = G[i, k].copy()
            for m in range(k):
                s = s - u[m] * Lm[k, m]
            u[k] = s
            Lm[i, k] = s / D[k]
            dd = dd - s * Lm[i, k]
        D[i] = dd
        ratios[i] = np.where(alive, dd / G[i, i], np.nan)
        alive = alive & (dd > ft(rcond_min) * G[i, i])
        nu[alive] = i + 1
    y = np.zeros((K, nt), dtype=ft)
    c = np.zeros((K, nt), dtype=ft)
    for i in range(K):
        s = b[i].copy()
        for m in range(i):
            s = s - Lm[i, m] * y[m]
        y[i] = s
    for i in range(K - 1, -1, -1):
        s = y[i] / D[i]
        for m in range(i + 1, K):
            s = np.where(m < nu, s - Lm[m, i] * c[m], s)
        c[i] = np.where(i < nu, s, ft(0.0))
    np.seterr(**err)
    return c, nu, ratios


def filter(d, modes, grp_start=None, wfit=None, rcond_min=1e-10, dtype=np.float64, phases=None):
    ft = dtype
    assert phases is None or dtype is np.float64
    d = np.asarray(d, dtype=np.float64)
    nd, nt = d.shape
    F = np.asarray(modes, dtype=np.float64).reshape(nd, -1).astype(ft)
    K = F.shape[1]
    groups = clamp_groups([0, nd] if grp_start is None else grp_start, nd)
    out = d.astype(ft)
    amps = np.zeros((len(groups), K, nt), dtype=ft)
    n_used = np.zeros((len(groups), nt), dtype=np.int64)
    ratios = np.full((len(groups), K, nt), np.nan, dtype=ft)
    with np.errstate(all="ignore"):
        for g, (lo, hi) in enumerate(groups):
            if hi == lo:
                continue
            w = np.ones((hi - lo, nt), dtype=ft) if wfit is None else np.asarray(wfit[lo:hi]).astype(ft)
            live = w > 0
            dv = d[lo:hi].astype(ft)
            Fg = F[lo:hi]
            G = np.zeros((K, K, nt), dtype=ft)
            b = np.zeros((K, nt), dtype=ft)
            for i in range(K):
                wf = w * Fg[:, i:i + 1]
                for k in range(i + 1):
                    G[i, k] = G[k, i] = _sum(wf * Fg[:, k:k + 1], live, ft, phases)
                b[i] = _sum(wf * dv, live, ft, phases)
            c, nu, r = solve(G, b, rcond_min, ft)
            amps[g], n_used[g], ratios[g] = c, nu, r
            f = c[0][None, :] * Fg[:, 0:1]
            for k in range(1, K):
                f = f + c[k][None, :] * Fg[:, k:k + 1]
            out[lo:hi] = np.where(nu[None, :] == 0, dv, dv - f)
    return Fit(out, amps, n_used, ratios)


projector = fit_ref.projector           # of one full-rank column of n detectors
