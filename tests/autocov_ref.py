"""numpy yardstick of the gappy autocovariance, CPU only: pxl_tod_autocov_f64 / pj.autocov_tod.

THE DEFINITION (include/pixell_hip.h).  Segments and LIVE are the Toeplitz weight's (toeplitz_ref.live_mask, fit_ref.clamp).
z = x at the live samples and +0.0 elsewhere.  sums[r][k] = sum of z_t z_(t+k) over the t with t and t + k live in the same segment,
pairs[r][k] the number of those t.

THE ORDER (csrc/pxl_autocov.h), which sums() restates operation by operation so that in Float64 it is the device bit for bit:
plan(lam) gives LPG, W = 5 LPG and P = 256 / LPG.  A segment [lo, hi) is walked in tiles of TILE = 1280 samples from lo; the
sample lo + u belongs to partial p = (u mod TILE) // W.  Each of the P partials starts from +0.0 and takes the terms of its samples
one by one, v_p = v_p + z_t * z_(t+k), segments in the order of s, a segment in the order of t, z_(t+k) = +0.0 from hi on (such a
term is +-0.0 and changes no bit of a finite sum; the device leaves most of them out).  Then for off = P/2, P/4 .. 1:
v_p = v_p + v_(p+off) for p < off; sums = v_0.  The loop below runs over t and is vectorised over the detectors and the lags, which
are independent sums.

bound() is (pairs_k + 2) 2^-52 sum |z_t z_(t+k)|: n once-rounded products summed in any order stay within n 2^-53 sum |terms| of the
exact sum to first order; the bound is twice that."""
import numpy as np

import fit_ref
import toeplitz_ref as TR

EPS = 2.0 ** -52
TILE = 1280                                                     # PXL_ACOV_C of csrc/pxl_autocov.h
LAMBDA_MAX = 4096


def plan(lam):
    """(LPG, W, P) of the device for this lambda."""
    need = (lam + 5) // 5
    lpg = 1
    while lpg < 256 and lpg < need:
        lpg *= 2
    return lpg, 5 * lpg, 256 // lpg


FORM_EDGES = tuple(sorted({lam for lpg in (1, 2, 4, 8, 16, 32, 64, 128) for lam in (5 * lpg - 1, 5 * lpg)} |
                          {lam for g in (1, 2, 3) for lam in (1280 * g - 1, 1280 * g)}))
"""The last lambda of every (LPG, number of lag groups) of the device and the first of the next."""


def sums(x, lam, seg, wlive=None, dtype=np.float64, absolute=False):
    """(D, lam + 1) of the definition in the device's order, in `dtype`; absolute: of |z| (for bound)."""
    x = np.asarray(x, dtype=np.float64)
    nd, nt = x.shape
    _lpg, W, P = plan(lam)
    live = TR.live_mask(x.shape, seg, wlive)
    v = np.zeros((nd, P, lam + 1), dtype=dtype)
    with np.errstate(all="ignore"):
        for lo, hi in fit_ref.clamp(seg, nt):
            L = hi - lo
            if L == 0:
                continue
            z = np.zeros((nd, L + lam + 1), dtype=dtype)
            zin = np.where(live[:, lo:hi], x[:, lo:hi], 0.0).astype(dtype)     # an x under a cut enters no arithmetic
            z[:, :L] = np.abs(zin) if absolute else zin
            for u in range(L):
                p = (u % TILE) // W
                v[:, p, :] = v[:, p, :] + z[:, u:u + 1] * z[:, u:u + lam + 1]
        off = P // 2
        while off >= 1:
            v[:, :off, :] = v[:, :off, :] + v[:, off:2 * off, :]
            off //= 2
    return v[:, 0, :]


def pairs(shape, lam, seg, wlive=None):
    """(D, lam + 1) int64: the number of pairs of live samples of one segment at every lag."""
    nd, nt = shape
    live = TR.live_mask(shape, seg, wlive).astype(np.int64)
    out = np.zeros((nd, lam + 1), dtype=np.int64)
    for lo, hi in fit_ref.clamp(seg, nt):
        g = live[:, lo:hi]
        for k in range(min(lam + 1, hi - lo)):
            out[:, k] += (g[:, :hi - lo - k] * g[:, k:]).sum(axis=1)
    return out


def bound(x, lam, seg, wlive=None):
    """(pairs_k + 2) 2^-52 sum |z_t z_(t+k)|, (D, lam + 1) Float64."""
    return (pairs(np.shape(x), lam, seg, wlive) + 2) * EPS * sums(x, lam, seg, wlive, np.float64, True)
