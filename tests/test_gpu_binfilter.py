"""The binned-template filter on the device: pxl_tod_binfilter_f64 and pj.binfilter_tod against the numpy yardstick
tests/binfilter_ref.py on the layouts of tests/binfilter_layouts.py, which states the accuracy clause and which inputs enter it.

BITS.  On every layout out, means and n_used equal the yardstick in the device's order (binfilter_ref.filter(lanes=G)) bit for bit.
No input is set aside here.
ACCURACY.  On the layouts admitted on the CPU (at most one in ten is not: tests/test_binfilter_ref.py) the device meets
e_dev <= 4 max_item(e_np) + 2^-52 max_item|d| against long double, for out and for the means in their own scale.

Measured on the MI355X when written: the bits on all 21 layouts; worst e_dev / bound on the admitted ones 0.998 (200 bins of 25 samples
on 32 lanes), 0.95 and 0.74 next, below 0.25 with 64 or 256 lanes; the one layout set aside, scan_run2, at 1.225 in numpy and on the
device alike.

Every raw call here goes through buffers with sentinels on both sides of out, means and n_used, which must stay intact."""
import numpy as np
import pytest
import torch
from gpu_support import dev, run_filter_entry, to_dev

import binfilter_layouts as BL
import binfilter_ref as BF
from conftest import bits_equal

pytestmark = pytest.mark.gpu

LAYOUTS = BL.layouts()


def run(pj, dev, d, order, bin_start, w=None, in_place=False, fit_info=True):
    """One call of the raw entry on sentinel-padded buffers.  order and bin_start are uploaded as they are (no host check).  Returns
    a binfilter_ref.Fit."""
    nd, nt = np.shape(d)
    nbin = len(bin_start) - 1
    head = [nd, nt, nbin, np.array([int(v) for v in bin_start], dtype=np.int64), np.array([int(v) for v in order], dtype=np.int64)]
    out, me, nu = run_filter_entry(pj, dev, "pxl_tod_binfilter_f64", head, d, w, nd * nbin, nd * nbin, in_place, fit_info)
    return BF.Fit(out, me.reshape(nd, nbin), nu.reshape(nd, nbin))


def same(a, b):
    return bits_equal(a.out, b.out) and bits_equal(a.means, b.means) and np.array_equal(a.n_used, b.n_used)


@pytest.mark.parametrize("k", range(len(LAYOUTS)), ids=[lay[0] for lay in LAYOUTS])
def test_layouts_against_the_yardstick(pj, dev, k):
    name, nd, nt, order, bin_start = LAYOUTS[k]
    refs = BL.case(k)
    d, w = refs.d, refs.w
    got = run(pj, dev, d, order, bin_start, w)
    assert same(got, refs.lanes)                                                 # the bits: nothing is set aside
    bad, worst = refs.clause(got)
    print("%s: G = %d, admitted %s, worst e_dev / bound = %.3f" % (name, refs.G, refs.admitted, worst))
    if refs.admitted:
        assert bad is None, bad
    assert bits_equal(got.means[got.n_used == 0], np.zeros(int((got.n_used == 0).sum())))
    inside = np.zeros(nt, dtype=bool)
    for t in refs.bins:
        inside[t] = True
    assert bits_equal(got.out[:, ~inside], d[:, ~inside])                        # the samples in no bin are copied
    # exact properties on the same inputs: a second call, in place, and without the fit's outputs
    assert same(run(pj, dev, d, order, bin_start, w), got)
    assert bits_equal(run(pj, dev, d, order, bin_start, w, in_place=True).out, got.out)
    assert bits_equal(run(pj, dev, d, order, bin_start, w, fit_info=False).out, got.out)


def test_a_plan_that_runs_outside_stays_inside_the_buffers(pj, dev):
    """Built by hand for the raw entry, on the sentinel-padded 3 x 130 of run().  Non-decreasing offsets that start below 0 and run
    past n_t are clamped: the yardstick's items.  An order with entries -1, n_t and 2^40 skips those positions, in both passes: the
    yardstick's again, and their samples, which no position names, keep what out held.  Offsets in any order and an order with a
    repeated entry give values the header leaves open: the call must stay inside its buffers and leave every sample finite."""
    nd, nt = 3, 130
    d, w = BL.make_data(nd, nt, 77)
    order, _b = BF.plan(BL.triangle(nt, 4, 52), 4)
    starts = [-5, 40, 200, 2 ** 62]
    got = run(pj, dev, d, order, starts, w)
    assert same(got, BF.filter(d, order, starts, wfit=w, lanes=BF.group(nt, 3)))
    holes = order.copy()
    at = [3, 50, 129]
    holes[at] = [-1, nt, 2 ** 40]
    starts = [0, 30, 70, 130]
    for in_place in (False, True):
        got = run(pj, dev, d, holes, starts, w, in_place=in_place)
        ref = BF.filter(d, holes, starts, wfit=w, lanes=BF.group(nt, 3))
        named = np.ones(nt, dtype=bool)
        named[order[at]] = False
        assert bits_equal(got.out[:, named], ref.out[:, named]) and bits_equal(got.means, ref.means) and np.array_equal(got.n_used, ref.n_used)
        if in_place:
            assert bits_equal(got.out[:, ~named], d[:, ~named])                  # not read, not written
    twice = order.copy()
    twice[10], twice[100] = twice[11], twice[5]
    for o, s in ((twice, [0, 30, 70, 130]), (order, [90, -2 ** 62, 2 ** 62, 17, 150, -1, 60, -2 ** 63, 2 ** 63 - 1, 0]), (holes, [2 ** 62, -7, 131, 3])):
        wild = run(pj, dev, d, o, s, w)
        assert np.isfinite(wild.out).all() and np.isfinite(wild.means).all() and ((wild.n_used == 0) | (wild.n_used == 1)).all()


def test_truncated_fits(pj, dev):
    """Bins of 40 samples with 0 and 1 live samples and one whose weights sum to +Inf: n_used is 0, 1 and 0; the first and the last are
    copied by bits, the live sample of the second comes out +0.0."""
    L = 40
    rng = np.random.default_rng(31)
    d = rng.normal(size=(2, 3 * L))
    w = np.zeros_like(d)
    w[:, L + 7] = 2.0                                                            # a power of two: (w d) / w is d exactly
    w[:, 2 * L + 5], w[:, 2 * L + 9], w[:, 2 * L + 11] = np.inf, 1.0, 2.0
    index = np.tile(np.arange(3), L)                                             # the three bins interleave in time
    order, bin_start = BF.plan(index, 3)
    spread = lambda a: np.concatenate([a[:, b * L:(b + 1) * L][:, :, None] for b in range(3)], axis=2).reshape(2, 3 * L)
    ds, ws = spread(d), spread(w)
    got = run(pj, dev, ds, order, bin_start, ws)
    assert same(got, BF.filter(ds, order, bin_start, wfit=ws, lanes=BF.group(3 * L, 3)))
    assert np.array_equal(got.n_used, [[0, 1, 0]] * 2) and bits_equal(got.means[:, [0, 2]], np.zeros((2, 2)))
    assert bits_equal(got.out[:, index != 1], ds[:, index != 1])
    assert bits_equal(got.out[:, index == 1][:, 7], np.zeros(2)) and bits_equal(got.means[:, 1], d[:, L + 7])


@pytest.mark.parametrize("nt,n_bin,period", [(130, 4, 52), (5000, 4, 160)], ids=["wave", "block"])
def test_exact_properties(pj, dev, nt, n_bin, period):
    nd = 2
    d, w = BL.make_data(nd, nt, 5)
    index = BL.triangle(nt, n_bin, period, turn=0.03)
    order, bin_start = BF.plan(index, n_bin)
    base = run(pj, dev, d, order, bin_start, w)
    # a null wfit is an array of ones
    assert same(run(pj, dev, d, order, bin_start, None), run(pj, dev, d, order, bin_start, np.ones_like(d)))
    # wfit times 2^k: the same out and means; d times 2^k: both scaled exactly
    for k in (3, -5):
        assert same(run(pj, dev, d, order, bin_start, w * 2.0 ** k), base)
        sd = run(pj, dev, d * 2.0 ** k, order, bin_start, w)
        assert bits_equal(sd.out, base.out * 2.0 ** k) and bits_equal(sd.means, base.means * 2.0 ** k)
    # the Python wrapper is the same call: the plan pair, an index with n_bin, (D, T) weights, one weight per detector, in place, the fit
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    plan = pj.bin_plan(index, n_bin)
    assert np.array_equal(plan[0].numpy(), order) and np.array_equal(plan[1].numpy(), bin_start)
    out, me, nu = pj.binfilter_tod(t(d), plan, w=t(w), return_fit_info=True)
    assert bits_equal(out.cpu().numpy(), base.out) and bits_equal(me.cpu().numpy(), base.means) and np.array_equal(nu.cpu().numpy(), base.n_used)
    on_dev = pj.bin_plan(t(index), n_bin)
    assert on_dev[0].device == dev and np.array_equal(on_dev[0].cpu().numpy(), order) and np.array_equal(on_dev[1].cpu().numpy(), bin_start)
    assert bits_equal(pj.binfilter_tod(t(d), on_dev, w=t(w)).cpu().numpy(), base.out)
    for ix in (index, t(index), torch.from_numpy(index)):
        assert bits_equal(pj.binfilter_tod(t(d), ix, n_bin=n_bin, w=t(w)).cpu().numpy(), base.out)
    wdet = np.array([0.5, 3.0])
    per_det = run(pj, dev, d, order, bin_start, np.repeat(wdet[:, None], nt, axis=1))
    buf = t(d)
    assert pj.binfilter_tod(buf, plan, w=t(wdet), out=buf) is buf
    assert bits_equal(buf.cpu().numpy(), per_det.out)
    # out may be tod itself and may not overlap it otherwise: one sample further into a common allocation is refused
    arena = torch.zeros((nd * nt + 1,), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="overlap"):
        pj.binfilter_tod(arena[:nd * nt].view(nd, nt), plan, out=arena[1:].view(nd, nt))


def test_exact_inputs_give_the_exact_mean_by_bits(pj, dev):
    """Integer d, unit weights and bins hit a power-of-two number of times: no sum rounds and the division is exact, so the order of
    the adds cannot show and out is d minus the exact mean, on every group size."""
    rng = np.random.default_rng(9)
    for nt, n_bin, hits in ((128, 64, 2), (128, 16, 8), (128, 2, 64), (4096, 2, 2048), (4096, 4, 1024), (64, 64, 1)):
        index = rng.permutation(np.repeat(np.arange(n_bin), hits))
        assert len(index) == nt
        d = rng.integers(-8, 9, (2, nt)).astype(float)
        order, bin_start = BF.plan(index, n_bin)
        got = run(pj, dev, d, order, bin_start, None)
        mean = np.stack([d[:, index == b].sum(axis=1) / hits for b in range(n_bin)], axis=1)
        assert bits_equal(got.means, mean + 0.0) and bits_equal(got.out, d - mean[:, index]) and (got.n_used == 1).all(), (nt, n_bin)


@pytest.mark.parametrize("nd,nt,seg", [(2, 130, [3, 40, 64, 129]), (1, 5000, [0, 1200, 2500, 5000])], ids=["wave", "block"])
def test_contiguous_bins_are_the_polynomial_filter_at_order_zero_by_bits(pj, dev, nd, nt, seg):
    """An identity order and bins that are segments: binfilter_tod is polyfilter_tod(order=0, rcond_min=0) bit for bit, on the device."""
    d, w = BL.make_data(nd, nt, 21)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    plan = (torch.arange(nt, dtype=torch.int64), torch.tensor(seg, dtype=torch.int64))
    for wv in (w, None):
        mine = pj.binfilter_tod(t(d), plan, w=None if wv is None else t(wv), return_fit_info=True)
        poly = pj.polyfilter_tod(t(d), seg, 0, w=None if wv is None else t(wv), rcond_min=0.0, return_fit_info=True)
        assert bits_equal(mine[0].cpu().numpy(), poly[0].cpu().numpy()) and bits_equal(mine[1].cpu().numpy(), poly[1].cpu().numpy()[:, :, 0])
        assert np.array_equal(mine[2].cpu().numpy(), poly[2].cpu().numpy())


@pytest.mark.parametrize("nt,n_bin,period", [(130, 4, 52), (5000, 4, 160)], ids=["wave", "block"])
def test_locality(pj, dev, nt, n_bin, period):
    nd = 3
    d, w = BL.make_data(nd, nt, 50)
    index = BL.triangle(nt, n_bin, period)
    order, bin_start = BF.plan(index, n_bin)
    base = run(pj, dev, d, order, bin_start, w)
    det, b = 1, 1
    own = np.zeros((nd, nt), dtype=bool)
    own[det, index == b] = True
    at = np.flatnonzero(index == b)
    mid = at[len(at) // 2]
    keep = np.ones((nd, n_bin), dtype=bool)
    keep[det, b] = False
    # a change of d or of wfit inside one (detector, bin) leaves every other sample's bits
    d2, w2 = d.copy(), w.copy()
    d2[det, at] += 3.0
    w2[det, at] = np.roll(w[det, at], 5)
    for dv, wv in ((d2, w), (d, w2)):
        got = run(pj, dev, dv, order, bin_start, wv)
        assert bits_equal(got.out[~own], base.out[~own]) and not bits_equal(got.out[own], base.out[own])
        assert bits_equal(got.means[keep], base.means[keep])
    # a NaN under a zero weight stays in its own sample
    w0 = w.copy()
    w0[det, mid] = 0.0
    d_nan = d.copy()
    d_nan[det, mid] = np.nan
    fin, nan = run(pj, dev, d, order, bin_start, w0), run(pj, dev, d_nan, order, bin_start, w0)
    here = np.zeros((nd, nt), dtype=bool)
    here[det, mid] = True
    assert np.isnan(nan.out[det, mid]) and bits_equal(nan.out[~here], fin.out[~here]) and bits_equal(nan.means, fin.means)
    # a NaN at a live sample reaches exactly its bin of its detector
    w1 = w.copy()
    w1[det, mid] = 1.0
    live, ref = run(pj, dev, d_nan, order, bin_start, w1), run(pj, dev, d, order, bin_start, w1)
    assert np.isnan(live.out[own]).all() and bits_equal(live.out[~own], ref.out[~own]) and live.n_used[det, b] == 1
    assert np.isnan(live.means[det, b]) and bits_equal(live.means[keep], ref.means[keep])
    # an all-cut bin is copied: n_used = 0, the bits of d, -0.0 and NaN included
    wc, dc = w.copy(), d.copy()
    wc[det, at] = np.array([0.0, -1.0, np.nan])[np.arange(len(at)) % 3]
    dc[det, at[0]], dc[det, at[1]] = -0.0, np.nan
    cut = run(pj, dev, dc, order, bin_start, wc)
    assert cut.n_used[det, b] == 0 and bits_equal(cut.means[det, b], 0.0)
    assert bits_equal(cut.out[own], dc[own]) and np.signbit(cut.out[det, at[0]])
    other = ~own
    other[det, :] = False
    assert bits_equal(cut.out[other], base.out[other])
