"""The end-to-end case of the filter-and-bin map-maker, shared by the CPU and the GPU tests, and its numpy
yardstick: polyfilter_ref for the filter, nearest_ref for the binning, polsolve_ref for the block solve.

A 24 x 12 patch of 1 degree pixels.  ND = 4 detectors within 0.3 pixel of one boresight, at polarisation angles 0, 45, 90 and
135 degrees, raster along RA: NSWEEP = 24 sweeps of SWEEP = 48 samples, two sweeps per pixel row, left to right and back, the
boresight's position angle random per sample.  One segment per sweep.  The sky is zero except a 2 x 2 pixel source in the middle
of the patch (and of its sweeps).  Every (detector, sweep) carries a random polynomial of degree <= ORDER = 3 whose Legendre
coefficients are 10^3 times the source; there is no noise, and w is one weight per detector."""
import numpy as np

import nearest_ref
import pointing_ref
import polsolve_ref
import polyfilter_ref as PF

ND, NSWEEP, SWEEP, ORDER, DRIFT, RCOND_MIN = 4, 24, 48, 3, 1.0e3, 1e-3
NT = NSWEEP * SWEEP
SRC_ROWS, SRC_COLS = (5, 6), (11, 12)                       # 0-based rows and columns of the source's pixels
SRC_IQU = (1.0, 0.3, -0.2)


class Case:
    def __init__(self, pj, O, seed=1812):
        import torch
        deg = np.pi / 180
        self.O = O
        self.shape, self.wcs = pj.geometry([[12 * deg, -12 * deg], [-6 * deg, 6 * deg]], 1.0 * deg)
        assert tuple(self.shape) == (24, 12)
        nx, ny = self.shape
        rng = np.random.default_rng(seed)
        s, j = np.divmod(np.arange(NT), SWEEP)
        f = (j + rng.uniform(0, 1, NT)) / SWEEP
        x = np.where(s % 2 == 0, f, 1.0 - f) * nx + 0.5
        y = (s // 2) + 1.0 + rng.uniform(-0.2, 0.2, NT)
        sky = O.pix2sky(self.wcs, np.stack([x, y], axis=1), O.WRAP_NONE)
        psi = rng.uniform(0, np.pi, NT)
        t = torch.from_numpy
        self.q_bore = pj.quat_from_radec(t(sky[:, 0].copy()), t(sky[:, 1].copy()), t(psi)).contiguous()
        xi, eta = rng.uniform(-0.3, 0.3, ND) * deg, rng.uniform(-0.3, 0.3, ND) * deg
        centre = pj.quat_from_radec(0.0, 0.0, 0.0)
        self.q_det = pj.quat_mul(pj.quat_conj(centre), pj.quat_from_radec(t(xi), t(eta), t(np.arange(ND) * np.pi / 4))).contiguous()
        self.w_det = 10.0 ** rng.uniform(-0.5, 0.5, ND)
        self.seg_start = [k * SWEEP for k in range(NSWEEP + 1)]
        self.m0 = np.zeros((3, ny, nx))
        self.src = np.zeros((ny, nx), dtype=bool)
        for r in SRC_ROWS:
            for c in SRC_COLS:
                self.src[r, c] = True
        for p in range(3):
            self.m0[p][self.src] = SRC_IQU[p]
        self.fit_mask = np.where(self.src, 0.0, 1.0)
        e = pointing_ref.expand(self.q_bore.numpy(), self.q_det.numpy())
        self.sky, self.resp = np.stack([e["ra"], e["dec"]], axis=1), np.stack([e["q"], e["u"]], axis=1)
        signal = nearest_ref.sample_pol(O, self.wcs, self.shape, self.m0, self.sky, self.resp).reshape(ND, NT)
        coef = rng.normal(size=(ND, NSWEEP, ORDER + 1)) * DRIFT
        P = np.stack(PF.basis(SWEEP, ORDER), axis=0)                                # (ORDER + 1, SWEEP)
        self.tod = signal + np.einsum("dsk,kj->dsj", coef, P).reshape(ND, NT)
        self.w = np.repeat(self.w_det[:, None], NT, axis=1)

    def w_fit(self, masked):
        """w * [fit_mask at the sample's nearest pixel > 0] (an off-map sample samples +0.0), or w."""
        if not masked:
            return self.w
        at = nearest_ref.sample(self.O, self.wcs, self.shape, self.fit_mask[None], self.sky)
        return self.w * (np.asarray(at).reshape(ND, NT) > 0)

    def yardstick(self, masked):
        """(map (3, ny, nx), solved (ny, nx), filtered (D, T)) of the numpy composition."""
        nx, ny = self.shape
        filt = PF.filter(self.tod, self.seg_start, ORDER, wfit=self.w_fit(masked)).out
        (rhs, _k, _S), (w6, _k6, _S6) = nearest_ref.bin(self.O, self.wcs, self.shape, self.sky, self.resp, filt.reshape(-1), self.w.reshape(-1))
        x, _rc, info = polsolve_ref.solve(w6.reshape(6, -1), rhs.reshape(3, -1), RCOND_MIN)
        return x.reshape(3, ny, nx), info["ok"].reshape(ny, nx), filt

    def errors(self, m, solved):
        """(worst |m - m0| on the source's pixels, worst off them) over the solved pixels."""
        err = np.abs(np.asarray(m) - self.m0)
        return float(err[:, self.src & solved].max()), float(err[:, ~self.src & solved].max())
