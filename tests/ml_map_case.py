"""The end-to-end case of the correlated-noise ML map-maker, shared by the CPU and the GPU tests, with its dense
numpy solution (toeplitz_ref.MLSystem on nearest_ref's pixels).

A 16 x 10 patch of 1 degree pixels.  ND = 4 detectors within 0.3 pixel of one boresight, at polarisation angles 0, 45, 90 and 135
degrees, NT = 3000 samples in NSCAN = 3 scans of 1000, one segment per scan.  Scans 0 and 2 raster along RA, one pixel row per 100
samples, there and back; scan 1 rasters along DEC, one column per 62.5 samples: the scans cross, which is what lets a map-maker
tell a drift from the sky.  The boresight's position angle is random per sample, so every pixel sees many angles and every pixel
block's rcond is far above RCOND_MIN (asserted by the CPU test).  The sky is a random IQU map.  10 % of the samples are cut
(w = 0), and the timestream under a cut is NaN: a cut sample's value must never be read.  The noise, for the tests that add it,
is 1 / f: P(f) = SIGMA^2 (1 + (FKNEE / f)^2), drawn per detector and scan; the kernel is pj.noise_kernel_from_psd of that
spectrum at LAMBDA = 64, the same for every detector."""
import numpy as np

import nearest_ref
import pointing_ref
import toeplitz_ref as TR

ND, NSCAN, SCAN, LAMBDA, RCOND_MIN = 4, 3, 1000, 64, 1e-3
NT = NSCAN * SCAN
SIGMA, FKNEE, NFFT = 1.0, 0.02, 4096
CUT = 0.10
SEEDS = (11, 12, 13, 14, 15)


def psd(n_fft=NFFT, sigma=SIGMA, fknee=FKNEE, alpha=2.0):
    """The one-sided spectrum at rfftfreq(n_fft); the f = 0 bin takes the value of the first positive frequency."""
    f = np.fft.rfftfreq(n_fft)
    f[0] = f[1]
    return sigma ** 2 * (1.0 + (fknee / f) ** alpha)


def noise(rng, n, n_fft=NFFT):
    """n samples of the spectrum psd(n_fft): white noise coloured in the frequency domain, the first n of n_fft samples."""
    white = np.fft.rfft(rng.normal(size=n_fft))
    return np.fft.irfft(white * np.sqrt(psd(n_fft)), n=n_fft)[:n]


class Case:
    def __init__(self, pj, O, seed=2104):
        import torch
        deg = np.pi / 180
        self.O = O
        self.shape, self.wcs = pj.geometry([[8 * deg, -8 * deg], [-5 * deg, 5 * deg]], 1.0 * deg)
        assert tuple(self.shape) == (16, 10)
        nx, ny = self.shape
        rng = np.random.default_rng(seed)
        x, y = np.empty(NT), np.empty(NT)
        j = np.arange(SCAN)
        for s in range(NSCAN):
            sl = slice(s * SCAN, (s + 1) * SCAN)
            jit = rng.uniform(0, 1, SCAN)
            if s != 1:                                          # along RA: row r = j // 100, there and back
                r, f = np.divmod(j, SCAN // ny)
                f = (f + jit) / (SCAN // ny)
                x[sl] = np.where((r + s // 2) % 2 == 0, f, 1.0 - f) * nx + 0.5
                y[sl] = r + 1.0 + rng.uniform(-0.3, 0.3, SCAN)
            else:                                               # along DEC: column c = j * nx // SCAN, there and back
                cpos = j * nx / SCAN
                c = np.floor(cpos)
                f = cpos - c + jit * nx / SCAN
                x[sl] = c + 1.0 + rng.uniform(-0.3, 0.3, SCAN)
                y[sl] = np.where(c % 2 == 0, f, 1.0 - f) * ny + 0.5
        sky = O.pix2sky(self.wcs, np.stack([x, y], axis=1), O.WRAP_NONE)
        psi = rng.uniform(0, np.pi, NT)
        t = torch.from_numpy
        self.q_bore = pj.quat_from_radec(t(sky[:, 0].copy()), t(sky[:, 1].copy()), t(psi)).contiguous()
        xi, eta = rng.uniform(-0.3, 0.3, ND) * deg, rng.uniform(-0.3, 0.3, ND) * deg
        centre = pj.quat_from_radec(0.0, 0.0, 0.0)
        self.q_det = pj.quat_mul(pj.quat_conj(centre), pj.quat_from_radec(t(xi), t(eta), t(np.arange(ND) * np.pi / 4))).contiguous()
        self.seg_start = [k * SCAN for k in range(NSCAN + 1)]
        self.m0 = rng.normal(size=(3, ny, nx))
        e = pointing_ref.expand(self.q_bore.numpy(), self.q_det.numpy())
        self.sky, self.resp = np.stack([e["ra"], e["dec"]], axis=1), np.stack([e["q"], e["u"]], axis=1)
        self.signal = nearest_ref.sample_pol(O, self.wcs, self.shape, self.m0, self.sky, self.resp).reshape(ND, NT)
        self.w = (rng.uniform(0, 1, (ND, NT)) >= CUT).astype(np.float64)
        self.kernel = np.tile(pj.noise_kernel_from_psd(psd(), LAMBDA).numpy(), (ND, 1))
        self._system = None

    def tod(self, seed=None):
        """signal (+ 1/f noise of `seed`), NaN under the cuts."""
        d = self.signal.copy()
        if seed is not None:
            rng = np.random.default_rng(seed)
            for det in range(ND):
                for s in range(NSCAN):
                    d[det, s * SCAN:(s + 1) * SCAN] += noise(rng, SCAN)
        d[self.w == 0] = np.nan
        return d

    def system(self, kernel=None, w=None):
        """toeplitz_ref.MLSystem of the case; the one of the case's own kernel and cuts is built once."""
        if kernel is None and w is None:
            if self._system is None:
                self._system = TR.MLSystem(self.O, self.wcs, self.shape, self.sky, self.resp, self.kernel, self.seg_start, self.w, RCOND_MIN)
            return self._system
        return TR.MLSystem(self.O, self.wcs, self.shape, self.sky, self.resp, self.kernel if kernel is None else kernel, self.seg_start,
                           self.w if w is None else w, RCOND_MIN)

    def rms(self, m, solved):
        return float(np.sqrt(np.mean((np.asarray(m) - self.m0)[:, solved] ** 2)))


_case = {}


def case(pj, O):
    """The shared, unchanged case."""
    if "c" not in _case:
        _case["c"] = Case(pj, O)
    return _case["c"]
