"""The per-scan polynomial filter on the device: pxl_tod_polyfilter_f64 and pj.polyfilter_tod against the numpy
yardstick tests/polyfilter_ref.py, which holds the definition twice, in Float64 with sequential sums and in long double.

ACCURACY.  Per sample e_dev = |out_dev - out_ld| and e_np = |out_f64 - out_ld|; the device must meet
e_dev <= 4 max_segment(e_np) + 2^-52 max_segment|d|: it differs from the Float64 yardstick only in the order of the moment sums
(4 x is the margin expand_pointing's test gives a different summation order), and the second term is the one rounding of the final
subtraction.  The coefficients meet the same bar in their own scale (max over the segment's coefficients).  Before the device
runs, every long-double pivot ratio is asserted to lie above 10^3 rcond_min or below 10^-3 rcond_min, so that no accept/reject
decision hangs on rounding; n_used must then equal the yardstick's exactly.  A second condition on the inputs, also decided on the
CPU, is stated at `admitted`.  Beyond the clause the device must give, bit for bit, the Float64 yardstick evaluated in its own
summation order (polyfilter_ref.filter(lanes=G)).

Measured on the MI355X when written: worst e_dev / bound 0.81 (order 3, segments of 8 samples on 2 lanes), 0.31 at worst with 64 or
256 lanes; the bits of the device-order yardstick on every layout.

Every call here goes through buffers with sentinels on both sides of out, coeffs and n_used, which must stay intact."""
import numpy as np
import pytest
import torch
from gpu_support import dev, run_filter_entry, steps as _steps

import polyfilter_ref as PF
from conftest import bits_equal

pytestmark = pytest.mark.gpu

ORDERS = (0, 1, 3, 7)
RCOND_MIN = 1e-10


def layouts(order):
    """(name, D, T, seg_start) for one order.  Segment lengths 1, 2, order + 1, order + 2, 63, 64, 65, 257, 1023, 1024 and 5000; gaps
    before the first and after the last segment; an empty segment; between them every group size the host can choose (asserted
    below), lanes that make one trip, two and twenty."""
    return [
        ("one_sample", 1, 1, [0, 1]),
        ("short", 3, 130, _steps([1, 2, order + 1, order + 2, 0, 63, 7], start=2)),       # gaps of 2 and of 130 - 85 - 2 o ... samples
        ("ones", 3, 130, list(range(131))),                                              # mean length 1: one lane per segment
        ("pairs", 3, 130, list(range(0, 131, 2))),
        ("fours", 3, 130, _steps([4] * 32, start=1)),
        ("eights", 3, 130, _steps([8] * 16)),
        ("sixteens", 3, 130, _steps([16] * 8, start=2)),
        ("wave", 3, 130, [0, 64, 129]),                                                  # 64 and 65
        ("block_1024", 2, 1100, [38, 1062]),                                             # one block per segment, gaps on both sides
        ("wave_1023", 2, 1100, [0, 1023, 1100]),                                         # 1023 samples on at most 64 lanes: 16 trips
        ("wave_257", 2, 1100, [10, 267, 1100]),
        ("block_5000", 1, 5000, [0, 5000]),                                              # 20 samples per lane of a block
        ("block_mixed", 1, 5000, [0, 257, 1280, 2304, 5000]),                            # 257, 1023, 1024 and 2696 on a block each
    ]


ALL = [(order, lay) for order in ORDERS for lay in layouts(order)]
IDS = ["o%d-%s" % (order, lay[0]) for order, lay in ALL]


def run(pj, dev, d, seg, order, w=None, rcond_min=RCOND_MIN, in_place=False, fit_info=True):
    """One call of the raw entry on sentinel-padded buffers.  seg is uploaded as it is (no host check).  Returns a polyfilter_ref.Fit
    (ratios None)."""
    nd, nt = np.shape(d)
    nseg = len(seg) - 1
    head = [nd, nt, nseg, np.array([int(v) for v in seg], dtype=np.int64), order, rcond_min]
    out, co, nu = run_filter_entry(pj, dev, "pxl_tod_polyfilter_f64", head, d, w, nd * nseg * (order + 1), nd * nseg, in_place, fit_info)
    return PF.Fit(out, co.reshape(nd, nseg, order + 1), nu.reshape(nd, nseg), None)


def make_data(nd, nt, seed, cut=0.1):
    """Noise of rms 1 on a slow drift of amplitude 100, weights in [0.5, 2) with a fraction `cut` of exact zeros."""
    rng = np.random.default_rng(seed)
    t = np.arange(nt) / max(nt, 2)
    d = rng.normal(size=(nd, nt)) + 100.0 * np.sin(3.0 * t + rng.uniform(0, 6, (nd, 1)))
    w = rng.uniform(0.5, 2.0, (nd, nt)) * (rng.uniform(0, 1, (nd, nt)) >= cut)
    return d, w


class Refs:
    """The three forms of the yardstick on one input: long double, Float64 with sequential sums, Float64 in the device's order."""

    def __init__(self, d, seg, order, w, rcond_min=RCOND_MIN):
        self.d, self.seg, self.order, self.w = d, [int(v) for v in seg], order, w
        self.G = PF.group(d.shape[1], len(seg) - 1, order)
        self.ld = PF.filter(d, seg, order, wfit=w, rcond_min=rcond_min, dtype=np.longdouble)
        r = np.asarray(self.ld.ratios, dtype=np.float64)
        r = r[~np.isnan(r)]
        self.decided = bool(((r > 1e3 * rcond_min) | (r < 1e-3 * rcond_min)).all())
        self.f64 = PF.filter(d, seg, order, wfit=w, rcond_min=rcond_min)
        self.lanes = self.f64 if self.G == 1 else PF.filter(d, seg, order, wfit=w, rcond_min=rcond_min, lanes=self.G)

    def clause(self, got):
        """The accuracy clause of the module's docstring for `got`: (the first violation or None, the worst e / bound)."""
        d, order = self.d, self.order
        nd, nt = d.shape
        ld, f64 = self.ld, self.f64
        if not (np.array_equal(got.n_used, ld.n_used) and np.array_equal(f64.n_used, ld.n_used)):
            return ("n_used",), np.inf
        worst, bad = 0.0, None
        for s, (lo, hi) in enumerate(PF.clamp_segments(self.seg, nt)):
            for det in range(nd):
                if hi == lo:
                    continue
                e_dev = np.abs(got.out[det, lo:hi] - ld.out[det, lo:hi]).astype(np.float64).max()
                e_np = np.abs(f64.out[det, lo:hi] - ld.out[det, lo:hi]).astype(np.float64).max()
                bound = 4 * e_np + 2.0 ** -52 * np.abs(d[det, lo:hi]).max()
                c_dev = np.abs(got.coeffs[det, s] - ld.coeffs[det, s]).astype(np.float64).max()
                c_np = np.abs(f64.coeffs[det, s] - ld.coeffs[det, s]).astype(np.float64).max()
                cbound = 4 * c_np + 2.0 ** -52 * float(np.abs(ld.coeffs[det, s]).max())
                if bad is None and not e_dev <= bound:
                    bad = ("out", s, det, e_dev, bound)
                if bad is None and not c_dev <= cbound:
                    bad = ("coeffs", s, det, c_dev, cbound)
                worst = max(worst, e_dev / bound, c_dev / cbound if cbound > 0 else 0.0)
        return bad, worst

    def check(self, got):
        """The device's result: the clause, the bits of the yardstick in the device's order, +0.0 past n_used and in empty segments,
        copies outside the segments.  Returns the worst e_dev / bound."""
        bad, worst = self.clause(got)
        assert bad is None, bad
        assert np.array_equal(got.n_used, self.lanes.n_used) and bits_equal(got.coeffs, self.lanes.coeffs) and bits_equal(got.out, self.lanes.out)
        past = np.arange(self.order + 1) >= got.n_used[:, :, None]
        assert bits_equal(got.coeffs[past], np.zeros(int(past.sum())))
        inside = np.zeros(self.d.shape[1], dtype=bool)
        for lo, hi in PF.clamp_segments(self.seg, self.d.shape[1]):
            inside[lo:hi] = True
        assert bits_equal(got.out[:, ~inside], self.d[:, ~inside])
        return worst


def admitted(build, seg, order, tries=64):
    """The first of the inputs build(0), build(1), ... that meets the two conditions on the INPUTS, both decided on the CPU from the
    yardstick alone before the device runs.  One: every long-double pivot ratio lies above 10^3 rcond_min or below 10^-3 rcond_min.
    Two: the Float64 yardstick summed in the device's order meets the accuracy clause.  The second is needed because, where a
    group has more than one lane, the clause compares two draws of one rounding distribution -- the sequential sums and the
    device's -- and on a short segment a draw is a few ulps of max|d|, with a few degrees of freedom: a CORRECT evaluation in
    the device's order exceeds 4 e_np + 2^-52 max|d| in about one input in twenty-five (11 of 272 layouts in a numpy trial over six
    seeds, orders 0 to 7, group sizes 2 to 16; none with 64 or 256 lanes, where the tree is the more accurate order).  An input
    where it does tests the draw, not the device.  The device is then held to the clause AND to the bits of that evaluation."""
    for k in range(tries):
        d, w = build(k)
        refs = Refs(d, seg, order, w)
        if refs.decided and refs.clause(refs.lanes)[0] is None:
            return refs
    raise AssertionError("no admissible input in %d tries" % tries)


def case(order, layout):
    _name, nd, nt, seg = layout
    return admitted(lambda k: make_data(nd, nt, 1000 * order + len(seg) + 7919 * k), seg, order)


def test_the_layouts_reach_every_group_size():
    seen = {PF.group(nt, len(seg) - 1, order) for order, (_n, _nd, nt, seg) in ALL}
    assert seen == {1, 2, 4, 8, 16, 32, 64, 256}
    lengths = {hi - lo for order, (_n, _nd, nt, seg) in ALL for lo, hi in PF.clamp_segments(seg, nt)}
    assert {0, 1, 2, 63, 64, 65, 257, 1023, 1024, 5000} <= lengths
    for order in ORDERS:
        assert {order + 1, order + 2} <= {hi - lo for o, (_n, _nd, nt, seg) in ALL if o == order for lo, hi in PF.clamp_segments(seg, nt)}


@pytest.mark.parametrize("order,layout", ALL, ids=IDS)
def test_layouts_against_the_yardstick(pj, dev, order, layout):
    name, nd, nt, seg = layout
    refs = case(order, layout)
    d, w = refs.d, refs.w
    got = run(pj, dev, d, seg, order, w)
    print("order %d %s: G = %d, worst e_dev / bound = %.3f" % (order, name, refs.G, refs.check(got)))
    # exact properties on the same inputs: a second call, in place, and without the fit's outputs
    again = run(pj, dev, d, seg, order, w)
    assert bits_equal(again.out, got.out) and bits_equal(again.coeffs, got.coeffs) and np.array_equal(again.n_used, got.n_used)
    assert bits_equal(run(pj, dev, d, seg, order, w, in_place=True).out, got.out)
    assert bits_equal(run(pj, dev, d, seg, order, w, fit_info=False).out, got.out)


@pytest.mark.parametrize("order", ORDERS)
def test_a_seg_start_that_runs_outside_is_clamped(pj, dev, order):
    """Built by hand for the raw entry.  Non-decreasing offsets that start below 0 and run past n_t are clamped: the yardstick's
    segments.  Offsets in any order, with ends below their starts and values near +-2^62, make overlapping segments whose values
    the header leaves open: the call must stay inside its buffers (run's sentinels) and copy or filter every sample to a finite
    value; nothing else is asked of it."""
    nd, nt = 3, 130
    seg = [-5, 40, 200, 2 ** 62]
    assert PF.clamp_segments(seg, nt) == [(0, 40), (40, 130), (130, 130)]
    refs = admitted(lambda k: make_data(nd, nt, 77 + order + 7919 * k), seg, order)
    refs.check(run(pj, dev, refs.d, seg, order, refs.w))
    wild = run(pj, dev, refs.d, [90, -2 ** 62, 2 ** 62, 17, 150, -1, 60, -2 ** 63, 2 ** 63 - 1, 0], order, refs.w)
    assert np.isfinite(wild.out).all() and ((wild.n_used >= 0) & (wild.n_used <= order + 1)).all()


def _few_live(order, k):
    """order + 2 detectors x 3 segments of 40 samples; detector n has n live samples per segment, at least 4 apart."""
    nd, L = order + 2, 40
    rng = np.random.default_rng(31 + order + 7919 * k)
    d = rng.normal(size=(nd, 3 * L))
    w = np.zeros_like(d)
    for n in range(nd):
        for s in range(3):
            live = s * L + np.sort(rng.choice(L // 4, size=n, replace=False)) * 4 + rng.integers(0, 4)
            w[n, live] = rng.uniform(0.5, 2.0, n)
    return d, w


@pytest.mark.parametrize("order", ORDERS)
def test_truncated_fits(pj, dev, order):
    """Segments with 0 .. order + 1 live samples among 40: n_used is the number of live samples, as the yardstick's."""
    nd, L = order + 2, 40
    seg = [0, L, 2 * L, 3 * L]
    refs = admitted(lambda k: _few_live(order, k), seg, order)
    got = run(pj, dev, refs.d, seg, order, refs.w)
    refs.check(got)
    assert np.array_equal(got.n_used, np.repeat(np.arange(nd)[:, None], 3, axis=1))
    assert bits_equal(got.out[0], refs.d[0])                                     # the detector with no live sample is copied


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nt,seg", [(130, [3, 64, 129]), (5000, [0, 2500, 5000])], ids=["wave", "block"])
def test_exact_properties(pj, dev, order, nt, seg):
    nd = 2
    d, w = make_data(nd, nt, 5 + order)
    base = run(pj, dev, d, seg, order, w)
    # a null wfit is an array of ones
    ones = run(pj, dev, d, seg, order, np.ones_like(d))
    none = run(pj, dev, d, seg, order, None)
    assert bits_equal(none.out, ones.out) and bits_equal(none.coeffs, ones.coeffs) and np.array_equal(none.n_used, ones.n_used)
    # wfit times 2^k: the same out and coeffs; d times 2^k: both scaled exactly
    for k in (3, -5):
        sw = run(pj, dev, d, seg, order, w * 2.0 ** k)
        assert bits_equal(sw.out, base.out) and bits_equal(sw.coeffs, base.coeffs) and np.array_equal(sw.n_used, base.n_used)
        sd = run(pj, dev, d * 2.0 ** k, seg, order, w)
        assert bits_equal(sd.out, base.out * 2.0 ** k) and bits_equal(sd.coeffs, base.coeffs * 2.0 ** k)
    # the Python wrapper is the same call: (D, T) weights, one weight per detector, in place, and the fit's outputs
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out, co, nu = pj.polyfilter_tod(t(d), seg, order, w=t(w), return_fit_info=True)
    assert bits_equal(out.cpu().numpy(), base.out) and bits_equal(co.cpu().numpy(), base.coeffs) and np.array_equal(nu.cpu().numpy(), base.n_used)
    wdet = np.array([0.5, 3.0])
    per_det = run(pj, dev, d, seg, order, np.repeat(wdet[:, None], nt, axis=1))
    buf = t(d)
    assert pj.polyfilter_tod(buf, torch.tensor(seg), order, w=t(wdet), out=buf) is buf
    assert bits_equal(buf.cpu().numpy(), per_det.out)
    # out may be tod itself and may not overlap it otherwise: one sample further into a common allocation is refused
    arena = torch.zeros((nd * nt + 1,), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="overlap"):
        pj.polyfilter_tod(arena[:nd * nt].view(nd, nt), seg, order, out=arena[1:].view(nd, nt))


def test_order_zero_on_exact_inputs_gives_the_yardsticks_bits(pj, dev):
    """Small-integer d and power-of-two weights: no sum rounds, so the order of the adds cannot show and the mean, its one division
    and the subtraction are the yardstick's bits, on every group size."""
    rng = np.random.default_rng(9)
    for name, nd, nt, seg in layouts(0):
        d = rng.integers(-8, 9, (nd, nt)).astype(float)
        w = 2.0 ** rng.integers(-2, 3, (nd, nt)) * (rng.uniform(0, 1, (nd, nt)) >= 0.1)
        ref = PF.filter(d, seg, 0, wfit=w)
        got = run(pj, dev, d, seg, 0, w)
        assert bits_equal(got.out, ref.out) and bits_equal(got.coeffs, ref.coeffs) and np.array_equal(got.n_used, ref.n_used), name


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nt,seg", [(130, [3, 40, 64, 129]), (5000, [0, 1200, 2500, 5000])], ids=["wave", "block"])
def test_locality(pj, dev, order, nt, seg):
    nd = 3
    d, w = make_data(nd, nt, 50 + order)
    base = run(pj, dev, d, seg, order, w)
    det, s = 1, 1
    lo, hi = seg[s], seg[s + 1]
    own = np.zeros((nd, nt), dtype=bool)
    own[det, lo:hi] = True
    mid = (lo + hi) // 2
    # a change of d or of wfit inside one (detector, segment) leaves every other sample's bits
    d2, w2 = d.copy(), w.copy()
    d2[det, lo:hi] += 3.0
    w2[det, lo:hi] = np.roll(w[det, lo:hi], 5)
    for dv, wv in ((d2, w), (d, w2)):
        got = run(pj, dev, dv, seg, order, wv)
        assert bits_equal(got.out[~own], base.out[~own]) and not bits_equal(got.out[own], base.out[own])
        keep = np.ones((nd, len(seg) - 1), dtype=bool)
        keep[det, s] = False
        assert bits_equal(got.coeffs[keep], base.coeffs[keep])
    # a NaN under a zero weight stays in its own sample
    w0 = w.copy()
    w0[det, mid] = 0.0
    d_nan = d.copy()
    d_nan[det, mid] = np.nan
    fin, nan = run(pj, dev, d, seg, order, w0), run(pj, dev, d_nan, seg, order, w0)
    here = np.zeros((nd, nt), dtype=bool)
    here[det, mid] = True
    assert np.isnan(nan.out[det, mid]) and bits_equal(nan.out[~here], fin.out[~here]) and bits_equal(nan.coeffs, fin.coeffs)
    # a NaN at a live sample makes exactly its own segment NaN
    w1 = w.copy()
    w1[det, mid] = 1.0
    live = run(pj, dev, d_nan, seg, order, w1)
    ref = run(pj, dev, d, seg, order, w1)
    assert np.isnan(live.out[own]).all() and bits_equal(live.out[~own], ref.out[~own])
    assert live.n_used[det, s] == ref.n_used[det, s]
    # an all-cut segment is copied: n_used = 0, the bits of d, -0.0 and NaN included
    wc, dc = w.copy(), d.copy()
    wc[det, lo:hi] = np.array([0.0, -1.0, np.nan])[np.arange(hi - lo) % 3]
    dc[det, lo], dc[det, lo + 1] = -0.0, np.nan
    cut = run(pj, dev, dc, seg, order, wc)
    assert cut.n_used[det, s] == 0 and bits_equal(cut.coeffs[det, s], np.zeros(order + 1))
    assert bits_equal(cut.out[own], dc[own]) and np.signbit(cut.out[det, lo])
    other = ~own
    other[det, :] = False
    assert bits_equal(cut.out[other], base.out[other])
