"""The end-to-end case of the template-and-bin map-maker, shared by the CPU and the GPU tests, and its numpy
yardstick: binfilter_ref for the filter, nearest_ref for the binning, polsolve_ref for the block solve.  Modelled on
filter_bin_case.py, whose patch, scan and detectors these are.

A 24 x 12 patch of 1 degree pixels.  ND = 4 detectors within 0.3 pixel of one boresight, at polarisation angles 0, 45, 90 and 135
degrees, raster along RA: NSWEEP = 24 sweeps of SWEEP = 48 samples, two sweeps per pixel row, left to right and back, the
boresight's position angle random per sample.  The sky is zero except a 2 x 2 pixel source in the middle of the patch.  The bin of a
sample is its phase along the sweep in NB = 12 steps of 4 samples, the two directions split: N_BIN = 24 bins of 48 samples each per
detector.  Every (detector, bin) carries its own constant -- ground pickup, fixed to the scan and not to the sky -- of 10^3 times the
source; there is no noise, and w is one weight per detector.  The fit mask is zero on the source."""
import numpy as np

import binfilter_ref as BF
import nearest_ref
import pointing_ref
import polsolve_ref

ND, NSWEEP, SWEEP, NB, PICKUP, RCOND_MIN = 4, 24, 48, 12, 1.0e3, 1e-3
NT, N_BIN = NSWEEP * SWEEP, 2 * NB
SRC_ROWS, SRC_COLS = (5, 6), (11, 12)                       # 0-based rows and columns of the source's pixels
SRC_IQU = (1.0, 0.3, -0.2)


class Case:
    def __init__(self, pj, O, seed=2014):
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
        # the phase along the sweep as the telescope sees it (left to right: j, back: SWEEP - 1 - j), and the direction
        self.index = (np.where(s % 2 == 0, j, SWEEP - 1 - j) // (SWEEP // NB) + NB * (s % 2)).astype(np.int64)
        self.order, self.bin_start = BF.plan(self.index, N_BIN)
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
        self.pickup = rng.normal(size=(ND, N_BIN)) * PICKUP
        self.tod = signal + self.pickup[:, self.index]
        self.w = np.repeat(self.w_det[:, None], NT, axis=1)
        live = self.w_fit(True) > 0
        assert not live.all(), "the mask cuts nothing: the case would not show that it matters"
        assert all(live[:, self.index == b].any(axis=1).all() for b in range(N_BIN)), "a bin has no live sample"

    def w_fit(self, masked):
        """w * [fit_mask at the sample's nearest pixel > 0] (an off-map sample samples +0.0), or w."""
        if not masked:
            return self.w
        at = nearest_ref.sample(self.O, self.wcs, self.shape, self.fit_mask[None], self.sky)
        return self.w * (np.asarray(at).reshape(ND, NT) > 0)

    def bin(self, filt):
        """(map (3, ny, nx), solved (ny, nx)) of the (D, T) Float64 timestream `filt`: nearest_ref.bin and polsolve_ref.solve."""
        nx, ny = self.shape
        (rhs, _k, _S), (w6, _k6, _S6) = nearest_ref.bin(self.O, self.wcs, self.shape, self.sky, self.resp, filt.reshape(-1), self.w.reshape(-1))
        x, _rc, info = polsolve_ref.solve(w6.reshape(6, -1), rhs.reshape(3, -1), RCOND_MIN)
        return x.reshape(3, ny, nx), info["ok"].reshape(ny, nx)

    def yardstick(self, masked, filtered=True):
        """(map, solved, filtered tod) of the numpy composition in Float64: with `filtered` binfilter_ref on the case's plan, fitted
        under the mask or not; without it the timestream as it is."""
        filt = self.tod
        if filtered:
            filt = BF.filter(self.tod, self.order, self.bin_start, wfit=self.w_fit(masked)).out
        return self.bin(filt) + (filt,)

    def errors(self, m, solved):
        """(worst |m - sky| on the source's pixels, worst off them) over the solved pixels."""
        err = np.abs(np.asarray(m) - self.m0)
        return float(err[:, self.src & solved].max()), float(err[:, ~self.src & solved].max())
