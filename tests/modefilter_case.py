"""The end-to-end case of the mode-filter-and-bin map-maker, shared by the CPU and the GPU tests, and its numpy
yardstick: modefilter_ref for the filter, nearest_ref for the binning, polsolve_ref for the block solve.  Modelled on
filter_bin_case.py.

A 24 x 12 patch of 1 degree pixels.  ND = 8 detectors in two groups of four, each group a row of detectors 1.6 pixels apart (so a
group spans 4.8 pixels, more than the source's diagonal: never is a whole group on the source), the two groups 0.3 pixel apart, at
polarisation angles k * 22.5 degrees; raster along RA: NSWEEP = 24 sweeps of SWEEP = 48 samples, two sweeps per pixel row, the
boresight's position angle random per sample.  The sky is zero except a 2 x 2 pixel source in the middle of the patch.  Every
group carries one common signal -- white, rms COMMON = 10^3 times the source -- that each detector sees through its own gain in
[0.5, 1.5]; there is no noise, and w is one weight per detector.  The fit mask is zero on the source; a sample is live where the
mask is > 0 at its nearest pixel (an off-map sample is not).  The case asserts that every time sample keeps at least K = 1 live
detector in each group, so that no column of the fit is truncated."""
import numpy as np

import modefilter_ref as MF
import nearest_ref
import pointing_ref
import polsolve_ref

ND, NSWEEP, SWEEP, COMMON, RCOND_MIN, K = 8, 24, 48, 1.0e3, 1e-3, 1
NT = NSWEEP * SWEEP
GRP_START = [0, 4, 8]
SRC_ROWS, SRC_COLS = (5, 6), (11, 12)                       # 0-based rows and columns of the source's pixels
SRC_IQU = (1.0, 0.3, -0.2)
POLY_ORDER = 0                                              # of the run without modes: one mean per detector and sweep


class Case:
    def __init__(self, pj, O, seed=1913):
        import torch
        deg = np.pi / 180
        self.O = O
        self.shape, self.wcs = pj.geometry([[12 * deg, -12 * deg], [-6 * deg, 6 * deg]], 1.0 * deg)
        assert tuple(self.shape) == (24, 12)
        nx, ny = self.shape
        rng = np.random.default_rng(seed)
        s, j = np.divmod(np.arange(NT), SWEEP)
        f = (j + rng.uniform(0, 1, NT)) / SWEEP
        x = np.where(s % 2 == 0, f, 1.0 - f) * (nx - 1) + 1.0        # the boresight stays half a pixel inside: a group across the scan keeps a detector on the map
        y = (s // 2) + 1.0 + rng.uniform(-0.2, 0.2, NT)
        sky = O.pix2sky(self.wcs, np.stack([x, y], axis=1), O.WRAP_NONE)
        psi = rng.uniform(0, np.pi, NT)
        t = torch.from_numpy
        self.q_bore = pj.quat_from_radec(t(sky[:, 0].copy()), t(sky[:, 1].copy()), t(psi)).contiguous()
        xi = np.tile(np.array([-2.4, -0.8, 0.8, 2.4]), 2) * deg
        eta = np.repeat(np.array([-0.15, 0.15]), 4) * deg
        centre = pj.quat_from_radec(0.0, 0.0, 0.0)
        self.q_det = pj.quat_mul(pj.quat_conj(centre), pj.quat_from_radec(t(xi), t(eta), t(np.arange(ND) * np.pi / 8))).contiguous()
        self.w_det = 10.0 ** rng.uniform(-0.5, 0.5, ND)
        self.gains = rng.uniform(0.5, 1.5, ND)
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
        common = rng.normal(size=(len(GRP_START) - 1, NT)) * COMMON
        self.tod = signal + self.gains[:, None] * np.repeat(common, np.diff(GRP_START), axis=0)
        self.w = np.repeat(self.w_det[:, None], NT, axis=1)
        live = self.w_fit(True) > 0
        for lo, hi in MF.clamp_groups(GRP_START, ND):
            assert (live[lo:hi].sum(axis=0) >= K).all(), "a time sample has fewer than K live detectors in a group"
        assert not live.all(), "the mask cuts nothing: the case would not show that it matters"

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

    def yardstick(self, filtered, dtype=np.float64):
        """(map, solved, filtered tod) of the numpy composition: with `filtered` the mode filter on the gains, fitted under the
        mask, in `dtype` (the binning and the solve are Float64 either way); without it the timestream as it is."""
        filt = self.tod
        if filtered:
            filt = np.asarray(MF.filter(self.tod, self.gains, GRP_START, wfit=self.w_fit(True), dtype=dtype).out, dtype=np.float64)
        return self.bin(filt) + (filt,)

    def errors(self, m, solved, truth=None):
        """(worst |m - truth| on the source's pixels, worst off them) over the solved pixels; truth: the sky."""
        err = np.abs(np.asarray(m) - (self.m0 if truth is None else truth))
        return float(err[:, self.src & solved].max()), float(err[:, ~self.src & solved].max())
