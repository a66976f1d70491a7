"""numpy / scipy yardstick for the normal operator y += P^T W P x (pxl_normal_car_pol_bilinear_f64 / pj.normal_pol) and for the
CG polarised map-maker on top of it (pj.pcg, pj.cg_map_pol), CPU only.

Nothing here is new arithmetic.  normal() is pol_ref.scatter of w * pol_ref.sample(...): the composition the device's contract
names, term for term, with scatter_ref's (ref, k, S) triple and its bound k * 2^-52 * S per pixel.  sparse_p() is the matrix of
P_pol from scatter_ref's taps (tap_ref.matrix, kept sparse), and the map-maker's yardstick is linear algebra on it: A = P^T W P,
its pixel blocks M, a direct solve, the extreme eigenvalues of the pencil (A, M).  tests/test_mapmaker_ref.py holds pj.pcg to
them on torch CPU tensors."""
import functools
import math

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import pol_ref
import polsolve_ref
import scatter_ref
import tap_ref


def normal(O, wcs, shape, x, sky, resp, w, out=None, row0=0, nrows=None):
    """The composition: pol_ref.scatter of w * pol_ref.sample(x).  x (3, ny, nx); out: the initial (3, ny, nx) map or None.
    Returns (ref, k, S) as tap_ref.accumulate forms them.  A point whose position is not finite has a NaN sample and no taps.
    With row0, nrows: x, out and the result hold rows [row0, row0 + nrows) of the full map, and a tap that is on the map but
    outside those rows raises."""
    if tap_ref.rows(shape, row0, nrows) != (0, int(shape[1])):          # scatter_ref.taps DROPS a tap outside the window: the device's rule
        tap_ref.window(scatter_ref.taps(O, wcs, shape, sky)[0], shape, row0, nrows, "raise", "bilinear tap")
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(w, dtype=np.float64) * pol_ref.sample(O, wcs, shape, x, sky, resp, row0=row0, nrows=nrows)
        return pol_ref.scatter(O, wcs, shape, sky, v, resp, out=out, row0=row0, nrows=nrows)


def sparse_p(O, wcs, shape, sky, resp):
    """P_pol as a scipy.sparse CSR matrix (N, 3 * ny * nx), from the taps pol_ref.dense uses: row k holds r_c[k] * w_t at column
    c * ny * nx + idx_t, r = (1, q, u).  Taps of one point that meet on one pixel add up."""
    idx, wt = scatter_ref.taps(O, wcs, shape, sky)
    return tap_ref.matrix(idx, wt, int(shape[0]) * int(shape[1]), resp, sparse=True)


# ---- the map-maker's cases: geometry, points per map (at least 48 per pixel) ------------------------------------------------------
POINTS = {"box_2x2": 2 * 10 ** 3, "box_5x7": 2 * 10 ** 4, "box_24x12": 6 * 10 ** 4, "cc_90x46": 2 * 10 ** 5}
SMALL = ("box_2x2", "box_5x7", "box_24x12")
MASKED_ROWS = (10.0, 36.0)          # the masked case: points only in these pixel rows of the (90, 46) map
RCOND_MIN = 1e-3


def geometries(pj):
    return tap_ref.geometries(pj, ("box_2x2", "box_5x7", "box_24x12", "cc_90x46", "box_80x40"))


def pixel_uniform(O, wcs, shape, n, rng, rows=None):
    """n points uniform in PIXEL space over [1, nx] x [1, ny] (x over the whole period of a full-circle map; y over `rows` if
    given), as (n, 2) of (ra, dec).  Not uniform on the sphere: every pixel of a full-sky map is hit equally often."""
    nx, ny = shape
    hi = nx + 1 if O.is_periodic(wcs, nx) else nx
    y0, y1 = (1.0, float(ny)) if rows is None else rows
    pix = np.stack([rng.uniform(1, hi, n), rng.uniform(y0, y1, n)], axis=1)
    return O.pix2sky(wcs, pix, O.WRAP_NONE)


class Case:
    """One least-squares problem: shape, wcs, sky, resp, w, m0, d0 = P m0 (noiseless), d = d0 + noise, and the linear algebra of it."""

    def __init__(self, pj, O, geom, n, seed, rows=None):
        self.geom = geom
        self.shape, self.wcs = geometries(pj)[geom]
        nx, ny = self.shape
        rng = np.random.default_rng(seed)
        self.sky = pixel_uniform(O, self.wcs, self.shape, n, rng, rows)
        psi = rng.uniform(0, np.pi, n)
        self.resp = np.stack([np.cos(2 * psi), np.sin(2 * psi)], axis=1)
        self.w = 10.0 ** rng.uniform(-1, 1, n)
        self.m0 = rng.normal(size=(3, ny, nx))
        self.P = sparse_p(O, self.wcs, self.shape, self.sky, self.resp)
        self.d0 = self.P @ self.m0.ravel()
        self.d = self.d0 + rng.normal(size=n) / np.sqrt(self.w)
        self.A = (self.P.T @ sp.diags(self.w) @ self.P).tocsr()
        self.w6 = pol_ref.scatter(O, self.wcs, self.shape, self.sky, self.w, self.resp, mode=1)[0].reshape(6, ny * nx)
        self.solved = polsolve_ref.solve(self.w6, np.zeros((3, ny * nx)), RCOND_MIN)[2]["ok"]          # (npix,)
        self.keep = np.flatnonzero(np.tile(self.solved, 3))                                         # indices into the 3 npix unknowns

    def rhs(self, d):
        return self.P.T @ (self.w * d)

    def minv(self, r):
        """M^-1 r, (3 npix,): polsolve_ref's block solve, +0.0 on unsolved pixels."""
        return polsolve_ref.solve(self.w6, np.asarray(r).reshape(3, -1), RCOND_MIN)[0].reshape(-1)

    def binned(self, d):
        return self.minv(self.rhs(d))

    def direct(self, d):
        """The least-squares map on the solved pixels by a sparse direct solve, +0.0 elsewhere, (3 npix,)."""
        x = np.zeros(self.A.shape[0])
        x[self.keep] = spl.spsolve(self.A[self.keep][:, self.keep].tocsc(), self.rhs(d)[self.keep])
        return x

    def anorm(self, e):
        e = np.asarray(e, dtype=np.float64).reshape(-1)
        return math.sqrt(float(e @ (self.A @ e)))

    @functools.cached_property
    def kappa(self):
        """lambda_max / lambda_min of the pencil (A, M) on the solved pixels, M the preconditioner's matrix: the 3 x 3 blocks the six
        weight planes hold (sum_k w_k wt_kp r r^T, the interpolation weight to the FIRST power: the lumped blocks a binned
        map-maker inverts, not A's own diagonal blocks, which carry wt_kp^2).  Dense scipy.linalg.eigh up to 1000 unknowns,
        Lanczos (largest; smallest by shift-invert at 0) beyond."""
        A = self.A[self.keep][:, self.keep]
        npix = self.shape[0] * self.shape[1]
        blocks = polsolve_ref.dense(self.w6)                                                        # (npix, 3, 3)
        pix = np.arange(npix)
        M = sp.coo_matrix((np.concatenate([blocks[:, a, b] for a in range(3) for b in range(3)]),
                           (np.concatenate([a * npix + pix for a in range(3) for b in range(3)]),
                            np.concatenate([b * npix + pix for a in range(3) for b in range(3)]))), shape=self.A.shape).tocsr()
        M = M[self.keep][:, self.keep]
        if A.shape[0] <= 1000:
            lam = scipy.linalg.eigh(A.toarray(), M.toarray(), eigvals_only=True)
            return float(lam[-1] / lam[0])
        A = A.tocsc()
        hi = spl.eigsh(A, k=1, M=M.tocsc(), which="LA", return_eigenvectors=False, tol=1e-8)[0]
        lo = spl.eigsh(A, k=1, M=M.tocsc(), sigma=0, which="LM", return_eigenvectors=False, tol=1e-8)[0]
        return float(hi / lo)


_cases = {}


def case(pj, O, geom, masked=False):
    """The shared, unchanged inputs of the CPU and GPU map-maker tests."""
    key = (geom, masked)
    if key not in _cases:
        if masked:
            assert geom == "cc_90x46"
            _cases[key] = Case(pj, O, geom, POINTS[geom], 77, rows=MASKED_ROWS)
        elif geom == "box_80x40":
            _cases[key] = Case(pj, O, geom, 2 * 10 ** 5, 78)
        else:
            _cases[key] = Case(pj, O, geom, POINTS[geom], 70 + len(geom))
    return _cases[key]


def iteration_cap(kappa, tol):
    """ceil(ln(2 sqrt(kappa) / tol) / ln((sqrt(kappa) + 1) / (sqrt(kappa) - 1))) + 5: the Chebyshev bound
    |e_k|_A <= 2 ((sqrt(kappa) - 1) / (sqrt(kappa) + 1))^k |e_0|_A carried into the stopping norm (a factor sqrt(kappa) between
    the A norm of the error and the M^-1 norm of the residual, both relative), plus five."""
    s = math.sqrt(kappa)
    return int(math.ceil(math.log(2 * s / tol) / math.log((s + 1) / (s - 1)))) + 5
