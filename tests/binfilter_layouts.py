"""The layouts on which the binned-template filter is held to its yardstick tests/binfilter_ref.py, their data on
committed seeds, and the accuracy clause -- shared by tests/test_binfilter_ref.py, which holds the yardstick alone to the cap on
the inputs set aside, and tests/test_gpu_binfilter.py, which runs the device.  No device is needed to import this.

ACCURACY.  Per sample e_dev = |out_dev - out_ld| and e_np = |out_f64 - out_ld|; the device must meet
e_dev <= 4 max_item(e_np) + 2^-52 max_item|d| per (detector, bin): it differs from the Float64 yardstick only in the order of the two
sums (4 x is the margin the other two filters give a different summation order), and the second term is the one rounding of the final
subtraction.  The means meet the same bar in their own scale, |c_dev - c_ld| <= 4 |c_np - c_ld| + 2^-52 |c_ld|.

THE INPUTS SET ASIDE.  The clause compares two draws of one rounding distribution, the sequential sums and the device's; on a short
item a draw is a few ulps of max|d|, and a CORRECT evaluation in the device's order can exceed the bar (a numpy trial of this
definition: 1 of 497 random bins, at worst 1.31 x the bar).  So a layout enters the accuracy check only if the Float64 yardstick
summed in the device's order (binfilter_ref.filter(lanes=G)) meets the clause: Refs.admitted, decided on the CPU before the device
runs.  At most one layout in ten may be set aside on the committed seeds (tests/test_binfilter_ref.py).  The bits check -- the device
equals the yardstick in its own order -- sets nothing aside."""
import functools

import numpy as np

import binfilter_ref as BF
import fit_ref

CUT = 0.2                                                   # one sample in five


def triangle(nt, n_bin, period, turn=0.0):
    """The bin index of a triangle-wave scan of `period` samples per there-and-back: the position x in [0, 1] binned into n_bin,
    -1 (filter nothing) where x is within `turn` of an end.  A sweep stays period / (2 n_bin) samples in a bin."""
    ph = (np.arange(nt) % period + 0.5) / period
    x = 1.0 - np.abs(2.0 * ph - 1.0)
    k = np.minimum(np.floor(x * n_bin).astype(np.int64), n_bin - 1)
    return np.where((x < turn) | (x > 1.0 - turn), -1, k)


def contiguous(lengths, before=0, after=0):
    """Bins that are consecutive runs of these lengths, with `before` and `after` samples in no bin."""
    return np.concatenate([np.full(before, -1), np.repeat(np.arange(len(lengths)), lengths), np.full(after, -1)]).astype(np.int64)


def _from_index(name, nd, index, n_bin):
    order, bin_start = BF.plan(index, n_bin)
    return name, nd, len(index), order, bin_start


def _identity(name, nd, nt, bin_start):
    return name, nd, nt, np.arange(nt, dtype=np.int64), np.array(bin_start, dtype=np.int64)


def layouts():
    """(name, D, T, order, bin_start).  D x T of 1 x 1, 3 x 130, 2 x 1100 and 1 x 5000; plans of a triangle-wave scan with runs of 1 to
    20 samples per bin, of a random index and of contiguous bins; every group size the host can choose; item lengths 0, 1, 2, 63,
    64, 65, 257, 1023, 1024 and 5000; lanes that make 1 to 20 trips; empty bins, a plan with every sample out of range, and samples in
    no bin both before bin_start[0] and after the last offset (all asserted in tests/test_binfilter_ref.py)."""
    rng = np.random.default_rng(2020)
    first_dropped = _from_index("first_bin_dropped", 3, triangle(130, 8, 48, turn=0.05), 8)
    return [
        _from_index("one_sample", 1, [0], 1),
        _from_index("random_ones", 3, rng.integers(0, 130, 130), 130),                   # G = 1, empty bins
        _from_index("scan_run1", 3, triangle(130, 65, 130), 65),                         # G = 2
        _from_index("random_fours", 3, rng.integers(-2, 34, 130), 32),                   # G = 4, some samples out of range
        _from_index("scan_run2", 3, triangle(130, 16, 64), 16),                          # G = 8
        _from_index("scan_run3_turns", 3, triangle(130, 8, 48, turn=0.05), 8),           # G = 16
        _from_index("lengths_1_2_63_64", 3, contiguous([1, 2, 63, 64]), 4),              # G = 32
        _from_index("scan_run6", 3, triangle(130, 4, 52), 4),                            # G = 32
        _from_index("wave_65_65", 3, contiguous([65, 65]), 2),                           # G = 64
        _from_index("random_halves", 3, rng.integers(0, 2, 130), 2),                     # G = 64
        _from_index("all_out_of_range", 3, np.full(130, -1), 4),
        first_dropped[:4] + (first_dropped[4][1:],),                                     # bin 0's samples stand before bin_start[0]: copied
        _identity("block_1024_gaps", 2, 1100, [38, 1062]),                               # G = 256, gaps on both sides
        _from_index("wave_257", 2, contiguous([257, 843]), 2),                           # G = 64: 5 and 14 trips
        _from_index("wave_1023", 2, contiguous([1023, 77]), 2),                          # 16 trips
        _from_index("scan_run5", 2, triangle(1100, 40, 400, turn=0.02), 40),             # G = 32
        _from_index("random_block", 2, rng.integers(0, 2, 1100) - 1, 1),                 # G = 256: half the samples in the one bin
        _from_index("scan_run20_block", 1, triangle(5000, 4, 160), 4),                   # G = 256
        _from_index("block_5000", 1, contiguous([5000]), 1),                             # 20 samples per lane of a block
        _from_index("random_block_4", 1, rng.integers(0, 4, 5000), 4),
        _from_index("scan_run5_long", 1, triangle(5000, 200, 2000), 200),                # G = 32
    ]


def make_data(nd, nt, seed, cut=CUT):
    """Noise of rms 1 on per-detector pickup of amplitude 100 that is smooth in time, weights in [0.5, 2) with a fraction `cut` of
    exact zeros."""
    rng = np.random.default_rng(seed)
    t = np.arange(nt) / max(nt, 2)
    d = rng.normal(size=(nd, nt)) + 100.0 * np.sin(3.0 * t + rng.uniform(0, 6, (nd, 1)))
    w = rng.uniform(0.5, 2.0, (nd, nt)) * (rng.uniform(0, 1, (nd, nt)) >= cut)
    return d, w


class Refs:
    """The three forms of the yardstick on one input: long double, Float64 with sequential sums, Float64 in the device's order."""

    def __init__(self, d, order, bin_start, w):
        self.d, self.order, self.bin_start, self.w = d, np.asarray(order, dtype=np.int64), np.asarray(bin_start, dtype=np.int64), w
        nt = d.shape[1]
        self.G = BF.group(nt, len(self.bin_start) - 1)
        self.ld = BF.filter(d, order, bin_start, wfit=w, dtype=np.longdouble)
        self.f64 = BF.filter(d, order, bin_start, wfit=w)
        self.lanes = self.f64 if self.G == 1 else BF.filter(d, order, bin_start, wfit=w, lanes=self.G)
        self.bins = [self.order[lo:hi] for lo, hi in fit_ref.clamp(self.bin_start, nt)]
        self.bins = [t[(t >= 0) & (t < nt)] for t in self.bins]
        self.admitted = self.clause(self.lanes)[0] is None

    def clause(self, got):
        """The accuracy clause of the module's docstring for `got`: (the first violation or None, the worst e / bound)."""
        d, ld, f64 = self.d, self.ld, self.f64
        if not (np.array_equal(got.n_used, ld.n_used) and np.array_equal(f64.n_used, ld.n_used)):
            return ("n_used",), np.inf
        worst, bad = 0.0, None
        for b, t in enumerate(self.bins):
            if len(t) == 0:
                continue
            for det in range(d.shape[0]):
                e_dev = np.abs(got.out[det, t] - ld.out[det, t]).astype(np.float64).max()
                e_np = np.abs(f64.out[det, t] - ld.out[det, t]).astype(np.float64).max()
                bound = 4 * e_np + 2.0 ** -52 * np.abs(d[det, t]).max()
                c_dev = float(abs(got.means[det, b] - ld.means[det, b]))
                cbound = 4 * float(abs(f64.means[det, b] - ld.means[det, b])) + 2.0 ** -52 * float(abs(ld.means[det, b]))
                if bad is None and not e_dev <= bound:
                    bad = ("out", b, det, e_dev, bound)
                if bad is None and not c_dev <= cbound:
                    bad = ("means", b, det, c_dev, cbound)
                worst = max(worst, e_dev / bound, c_dev / cbound if cbound > 0 else 0.0)
        return bad, worst


@functools.lru_cache(maxsize=None)
def case(k):
    """Refs of layout k on its committed seed, computed once per process and left unchanged."""
    _name, nd, nt, order, bin_start = layouts()[k]
    d, w = make_data(nd, nt, 4200 + k)
    return Refs(d, order, bin_start, w)
