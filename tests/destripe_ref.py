"""numpy yardstick for the destriper, CPU only: the two passes pj.baseline_bin_pol_nearest and
pj.baseline_project_pol_nearest operation by operation, their exact per-pixel and per-baseline sums, and the whole map-maker
pj.destripe_map_pol_nearest_tod on dense matrices.

The model is d = P m + F a + n: P the nearest-pixel polarised pointing matrix (nearest_ref gives the pixel), n white noise of
weights w, F one amplitude per detector and `blen` consecutive samples.  An observation is (D, T), n_base = ceil(T / blen), and
baseline b = det * n_base + t // blen.  A time chunk [t0, t0 + n_chunk) is detector-major: sample k has det = k // n_chunk,
j = k % n_chunk.

    sample value   x = d (a None), a[b] (d None), d - a[b] with one rounding (both)
    cut            the sample has no pixel (position not finite, off the map) or mask[pixel] is not > 0
    bin            per uncut sample v = w * x (one rounding), then pol_ref.terms(v, resp): the three adds of the scatter
    project        per uncut sample w * (x - s), s = pol_ref.combine of the map's three values at the pixel; w * x with no map

tests/test_destripe_ref.py holds the operator built from these to the dense F^T W Z F."""
import math

import numpy as np

import nearest_ref
import pol_ref
import polsolve_ref
import tap_ref

U53 = 2.0 ** -53


def n_base(nt, blen):
    return -(-int(nt) // int(blen))


class Chunk:
    """What both passes form per sample of one chunk: idx (the pixel, -1 for none), live (not cut), b (the baseline), x (the
    sample value; whatever d and a give at a cut sample, NaN included, it is never used)."""

    def __init__(self, O, wcs, shape, sky, w, nd, t0, blen, nb, d=None, a=None, mask=None, row0=0, nrows=None):
        assert d is not None or a is not None
        self.row0, self.nrows = tap_ref.rows(shape, row0, nrows)
        self.w = np.asarray(w, dtype=np.float64).reshape(-1)
        n = len(self.w)
        assert n % nd == 0
        nc = n // nd
        assert nc == 0 or (t0 + nc - 1) // blen < nb
        k = np.arange(n)
        det, j = (k // nc, k % nc) if nc else (k, k)
        self.b = det * nb + (t0 + j) // blen
        # idx: into the resident rows, which mask, m and out hold; a pixel outside raises
        self.idx = tap_ref.window(nearest_ref.taps(O, wcs, shape, sky)[0], shape, row0, nrows, "raise", "nearest pixel")
        self.live = self.idx >= 0
        if mask is not None:
            mv = np.asarray(mask, dtype=np.float64).reshape(-1)
            with np.errstate(invalid="ignore"):
                self.live = self.live & (mv[np.where(self.idx >= 0, self.idx, 0)] > 0)
        with np.errstate(invalid="ignore", over="ignore"):
            if a is None:
                self.x = np.asarray(d, dtype=np.float64).reshape(-1).copy()
            elif d is None:
                self.x = np.asarray(a, dtype=np.float64).reshape(-1)[self.b]
            else:
                self.x = np.asarray(d, dtype=np.float64).reshape(-1) - np.asarray(a, dtype=np.float64).reshape(-1)[self.b]
        self.nb_all = nd * nb


def bin_products(ch):
    """(v, live): v = w * x with one rounding at the uncut samples (0.0, unused, at the others)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(ch.live, ch.w * np.where(ch.live, ch.x, 0.0), 0.0), ch.live


def exact_sums(at, terms, size, init=None):
    """Per slot of `size`: (ref, k, S), ref the math.fsum of the slot's terms (exactly rounded), k their number and S the sum of
    their magnitudes, an initial value counted as a term.  NaN and Inf terms make the slot's ref whatever their plain sum is."""
    ref = np.zeros(size) if init is None else np.array(init, dtype=np.float64).reshape(size).copy()
    k = np.zeros(size, np.int64) if init is None else np.ones(size, np.int64)
    S = np.abs(ref)
    order = np.argsort(at, kind="stable")
    at_s, t_s = np.asarray(at)[order], np.asarray(terms, dtype=np.float64)[order]
    cuts = np.flatnonzero(np.diff(at_s)) + 1
    for lo, hi in zip(np.concatenate(([0], cuts)), np.concatenate((cuts, [len(at_s)]))):
        if hi == lo:
            continue
        p, t = at_s[lo], t_s[lo:hi]
        vals = ([ref[p]] if init is not None else []) + list(t)
        ref[p] = math.fsum(vals) if np.all(np.isfinite(vals)) else float(np.sum(vals))
        k[p] += hi - lo
        S[p] += np.abs(t).sum()
    return ref, k, S


def bin(O, wcs, shape, sky, resp, w, nd, t0, blen, nb, d=None, a=None, mask=None, out=None, row0=0, nrows=None):
    """The binning pass: (ref, k, S) per plane and pixel, (3, ny, nx) each, ref the exactly rounded sum of the pixel's terms.
    With row0, nrows: mask, out and the result hold rows [row0, row0 + nrows) of the full map (ny below is their number), and a
    sample whose pixel is on the map but outside them raises."""
    ch = Chunk(O, wcs, shape, sky, w, nd, t0, blen, nb, d, a, mask, row0, nrows)
    nx, ny = int(shape[0]), ch.nrows
    v, live = bin_products(ch)
    with np.errstate(invalid="ignore", over="ignore"):
        t = pol_ref.terms(v[live], np.asarray(resp, dtype=np.float64).reshape(-1, 2)[live], 0)
    planes = [exact_sums(ch.idx[live], t[c], ny * nx, None if out is None else np.asarray(out)[c]) for c in range(3)]
    return tuple(np.stack([p[i] for p in planes]).reshape(3, ny, nx) for i in range(3))


def project_terms(O, wcs, shape, sky, resp, w, nd, t0, blen, nb, d=None, a=None, m=None, mask=None, row0=0, nrows=None):
    """(terms, b) of the uncut samples in sample order: w * (x - s) with two roundings, or w * x with one when m is None."""
    ch = Chunk(O, wcs, shape, sky, w, nd, t0, blen, nb, d, a, mask, row0, nrows)
    live = ch.live
    x, wl = ch.x[live], ch.w[live]
    with np.errstate(invalid="ignore", over="ignore"):
        if m is not None:
            planes = np.asarray(m, dtype=np.float64).reshape(3, -1)[:, ch.idx[live]]
            x = x - pol_ref.combine(planes, np.asarray(resp, dtype=np.float64).reshape(-1, 2)[live])
        return wl * x, ch.b[live], ch.nb_all


def project(O, wcs, shape, sky, resp, w, nd, t0, blen, nb, d=None, a=None, m=None, mask=None, out=None, row0=0, nrows=None):
    """The projection pass: (ref, n, S, touched) per baseline, (nd * nb,) each: the exactly rounded sum of the baseline's terms
    added to out (zeros for None) with one more rounding, the number of terms, the sum of their magnitudes, and whether the
    baseline had an uncut sample here (where not, the device leaves out's bits alone).  With row0, nrows: m and mask hold rows
    [row0, row0 + nrows) of the full map, and a sample whose pixel is on the map but outside them raises."""
    terms, b, size = project_terms(O, wcs, shape, sky, resp, w, nd, t0, blen, nb, d, a, m, mask, row0, nrows)
    seg, n, S = exact_sums(b, terms, size)
    base = np.zeros(size) if out is None else np.asarray(out, dtype=np.float64).reshape(size)
    touched = n > 0
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(touched, base + seg, base), n, S, touched


def bin_bound(ref, k, S):
    """The scatters' clause, (k - 1) 2^-53 sum|term| against the exact sum, plus the one rounding of the exactly rounded ref."""
    return np.maximum(k - 1, 0) * U53 * S + U53 * np.abs(ref)


def project_bound(n, S):
    """n 2^-52 sum|term| per baseline against the math.fsum of its terms, for a call that starts from zeros (out[b] = +0.0 + sum is
    exact).  Every term is defined to the bit and only the order of the n - 1 adds is free: at most (n - 1) 2^-53 S (1 + O(2^-53 n))
    from them and 2^-53 S from the rounding of the fsum itself, together under n 2^-53 S (1 + ...) < n 2^-52 S."""
    return n * 2.0 ** -52 * S


# ---- the map-maker on dense matrices ---------------------------------------------------------------------------------------------------

class Dense:
    """The whole observation as one chunk: P (N x 3 npix), F (N x nd nb), W and the solved set of pol_block_solve's rule at
    rcond_min.  A sample on an unsolved pixel is cut: its rows of P and F and its weight are zero."""

    def __init__(self, O, wcs, shape, sky, resp, w, nd, nt, blen, rcond_min):
        self.O, self.wcs, self.shape, self.sky, self.resp = O, wcs, shape, np.asarray(sky), np.asarray(resp)
        self.nd, self.nt, self.blen, self.nb, self.rmin = nd, nt, blen, n_base(nt, blen), rcond_min
        nx, ny = shape
        self.w = np.broadcast_to(np.asarray(w, dtype=np.float64).reshape(nd, -1), (nd, nt)).reshape(-1).copy()
        (_r, _k, _S), (w6, _k6, _S6) = nearest_ref.bin(O, wcs, shape, sky, resp, np.zeros(nd * nt), self.w)
        self.w6 = w6.reshape(6, -1)
        _x, rc, info = polsolve_ref.solve(self.w6, np.zeros((3, ny * nx)), rcond_min)
        self.rcond, self.solved = rc.reshape(ny, nx), info["ok"].reshape(ny, nx)
        self.mask = self.solved.astype(np.float64)
        ch = Chunk(O, wcs, shape, sky, self.w, nd, 0, blen, self.nb, d=np.zeros(nd * nt), mask=self.mask)
        self.live, self.b = ch.live, ch.b

    def matrices(self):
        """(P, F, W, Z, A): cut rows zeroed; Z = I - P M^+ P^T W, A = F^T W Z F."""
        n = self.nd * self.nt
        P = nearest_ref.dense(self.O, self.wcs, self.shape, self.sky, self.resp) * self.live[:, None]
        F = np.zeros((n, self.nd * self.nb))
        F[np.flatnonzero(self.live), self.b[self.live]] = 1.0
        W = np.diag(np.where(self.live, self.w, 0.0))
        Z = np.eye(n) - P @ np.linalg.pinv(P.T @ W @ P, hermitian=True) @ P.T @ W
        return P, F, W, Z, F.T @ W @ Z @ F

    def _chunk_args(self):
        return self.O, self.wcs, self.shape, self.sky, self.resp, self.w, self.nd, 0, self.blen, self.nb

    def solve_map(self, d=None, a=None):
        """M^-1 P^T W x over the uncut samples: the binning pass, then polsolve_ref.solve against the weights."""
        y = bin(*self._chunk_args(), d=d, a=a, mask=self.mask)[0]
        return polsolve_ref.solve(self.w6, y.reshape(3, -1), self.rmin)[0].reshape(y.shape)

    def project(self, d=None, a=None, m=None):
        return project(*self._chunk_args(), d=d, a=a, m=m, mask=self.mask)[0]

    def apply(self, p):
        """A p the way the map-maker forms it: bin(a = p), the block solve, project(a = p, m = that)."""
        return self.project(a=p, m=self.solve_map(a=p))

    def destripe(self, pj, d, tol, maxiter):
        """The map-maker's steps with this file's passes and the package's own pcg on CPU tensors.  Returns (map, baselines
        (nd, nb), info)."""
        import torch
        d = np.asarray(d, dtype=np.float64).reshape(-1)
        b = self.project(d=d, m=self.solve_map(d=d))
        s = self.project(a=np.ones(self.nd * self.nb))

        def minv(r):
            with np.errstate(divide="ignore", invalid="ignore"):
                return torch.from_numpy(np.where(s > 0, r.numpy() / s, 0.0))

        a, info = pj.pcg(lambda p: torch.from_numpy(self.apply(p.numpy())), minv, torch.from_numpy(b), tol, maxiter)
        a = a.numpy()
        return self.solve_map(d=d, a=a), a.reshape(self.nd, self.nb), info


# ---- the end-to-end case of the CPU and GPU tests -------------------------------------------------------------------------------------

class Scan:
    """nd = 4 detectors follow one boresight over a 12 x 7 patch of 1 degree pixels for nt = 600 samples: the first half rasters
    along RA row by row, the second half along DEC column by column, so the two directions cross in every pixel.  The boresight
    is uniform in pixel space over the whole patch, its position angle is random per sample, and the detectors sit within half
    a pixel of it at angles 0, 45, 90 and 135 degrees: a few samples fall off the patch and are cut.  Offsets of rms 5 per
    (detector, baseline of 37 samples) are added to noiseless samples of a random sky; w is one weight per detector."""
    ND, NT, BLEN, OFFSET_RMS, RCOND_MIN, TOL, MAXITER = 4, 600, 37, 5.0, 1e-3, 1e-8, 200

    def __init__(self, pj, seed=417):
        import torch
        deg = np.pi / 180
        self.shape, self.wcs = pj.geometry([[6 * deg, -6 * deg], [-3.5 * deg, 3.5 * deg]], 1.0 * deg)
        assert tuple(self.shape) == (12, 7)
        nx, ny = self.shape
        rng = np.random.default_rng(seed)
        h = self.NT // 2
        f = (np.arange(h) + rng.uniform(0, 1, h)) / h                              # progress along each half, 0 to 1
        rows, cols = f * ny, f * nx
        x = np.concatenate(((rows % 1.0) * nx, np.floor(cols) + rng.uniform(0, 1, h))) + 0.5
        y = np.concatenate((np.floor(rows) + rng.uniform(0, 1, h), (cols % 1.0) * ny)) + 0.5
        self.pix = np.stack([x, y], axis=1)
        self.psi = rng.uniform(0, np.pi, self.NT)
        cell = 1.0 * deg
        self.det_xi, self.det_eta = rng.uniform(-0.5, 0.5, self.ND) * cell, rng.uniform(-0.5, 0.5, self.ND) * cell
        self.det_psi = np.arange(self.ND) * np.pi / 4
        self.w_det = 10.0 ** rng.uniform(-0.5, 0.5, self.ND)
        self.m0 = rng.normal(size=(3, ny, nx))
        self.nb = n_base(self.NT, self.BLEN)
        self.a0 = rng.normal(size=(self.ND, self.nb)) * self.OFFSET_RMS
        self._torch = torch

    def quaternions(self, pj, O):
        """(q_bore (T, 4), q_det (D, 4)) as CPU tensors, built with the package's host-side quaternion helpers."""
        t = self._torch
        sky = O.pix2sky(self.wcs, self.pix, O.WRAP_NONE)
        qb = pj.quat_from_radec(t.from_numpy(sky[:, 0].copy()), t.from_numpy(sky[:, 1].copy()), t.from_numpy(self.psi))
        centre = pj.quat_from_radec(0.0, 0.0, 0.0)
        qd = pj.quat_mul(pj.quat_conj(centre), pj.quat_from_radec(t.from_numpy(self.det_xi), t.from_numpy(self.det_eta), t.from_numpy(self.det_psi)))
        return qb.contiguous(), qd.contiguous()

    def tod(self, O, sky, resp, offsets=True):
        """(D, T): noiseless samples of m0 at the expanded (sky, resp), plus F a0."""
        d = nearest_ref.sample_pol(O, self.wcs, self.shape, self.m0, sky, resp).reshape(self.ND, self.NT)
        if offsets:
            d = d + np.repeat(self.a0, self.BLEN, axis=1)[:, :self.NT]
        return d

    def dense(self, O, sky, resp):
        return Dense(O, self.wcs, self.shape, sky, resp, self.w_det[:, None], self.ND, self.NT, self.BLEN, self.RCOND_MIN)


def map_error(m, m0, solved):
    """max |m - m0| over the solved pixels after the mean of I over them is removed from both (the gauge)."""
    m, m0 = np.array(m, dtype=np.float64), np.array(m0, dtype=np.float64)
    m[0] -= m[0][solved].mean()
    m0[0] -= m0[0][solved].mean()
    return float(np.abs(m - m0)[:, solved].max())
