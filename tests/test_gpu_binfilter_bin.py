"""pj.template_bin_map_pol_nearest_tod on the device, on tests/binfilter_case.py: filter_bin_case's 24 x 12
patch, 4 detectors and 24 sweeps, a zero sky with one compact source, and per-detector pickup that is constant on the bins of the
sweep phase, the two directions split, at 10^3 times the source; no noise.

The bar of the masked case is 4 x the error of the same pipeline evaluated in numpy Float64 -- binfilter_ref, then the nearest-pixel
binning yardstick and the block solve -- against the true sky, worst over the solved pixels: computed here on the CPU, not taken
from the device."""
import numpy as np
import pytest
import torch
from gpu_support import dev, to_dev

import binfilter_case as BC
from conftest import bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bc(pj, O):
    return BC.Case(pj, O)


def _n(e):
    return e.data.cpu().numpy() if hasattr(e, "data") and not isinstance(e, torch.Tensor) else e.cpu().numpy()


def _args(bc, dev, w=None):
    return (to_dev(bc.tod, dev), to_dev(bc.w if w is None else w, dev), bc.q_bore.to(dev), bc.q_det.to(dev), None, bc.shape, bc.wcs)


def _plan(bc, dev):
    return (torch.from_numpy(bc.order).to(dev), torch.from_numpy(bc.bin_start).to(dev))


def _make(pj, dev, bc, masked=True, with_bins=True, order=None, chunk_t=None, w=None, **kw):
    mask = pj.Enmap(to_dev(bc.fit_mask, dev), bc.wcs) if masked else None
    bins = kw.pop("bins", _plan(bc, dev) if with_bins else None)
    return pj.template_bin_map_pol_nearest_tod(*_args(bc, dev, w), bins, bc.seg_start if order is not None else None, order, fit_mask=mask,
                                               rcond_min=BC.RCOND_MIN, chunk_t=chunk_t, **kw)


def test_with_the_mask_and_the_bins_the_map_is_the_sky(pj, dev, bc):
    """The test that fails without the feature."""
    m_np, solved_np, _f = bc.yardstick(True)
    bar = 4 * max(bc.errors(m_np, solved_np))
    m, rcond, _weights, filt = _make(pj, dev, bc)
    solved = _n(rcond) >= BC.RCOND_MIN
    on, off = bc.errors(_n(m), solved)
    print("masked: numpy's error against the sky %.3g (bar %.3g); device on the source %.3g, off it %.3g" % (bar / 4, bar, on, off))
    assert solved.all() and solved_np.all()
    assert on <= bar and off <= bar
    # the filtered timestream is binfilter_tod of the timestream with the masked weights, in bits, and tod is not changed
    comp = pj.binfilter_tod(to_dev(bc.tod, dev), _plan(bc, dev), w=to_dev(bc.w_fit(True), dev))
    assert bits_equal(_n(filt), _n(comp))
    # an (index, n_bin) pair is the same plan
    again = _make(pj, dev, bc, bins=(bc.index, BC.N_BIN))
    assert bits_equal(_n(again[3]), _n(filt))


def test_negative_controls(pj, dev, bc):
    """Without bins (a mean per detector and sweep in its place: the map-maker has no run with no filter) the map is wrong by the
    order of the pickup; with bins and without the mask the source is biased low, by more than the bar."""
    m, rcond, _weights, _filt = _make(pj, dev, bc, with_bins=False, order=0)
    solved = _n(rcond) >= BC.RCOND_MIN
    worst = max(bc.errors(_n(m), solved))
    print("without bins: worst |map - sky| = %.3g" % worst)
    assert solved.all() and worst > 0.1 * BC.PICKUP
    m_np, solved_np, _f = bc.yardstick(True)
    bar = 4 * max(bc.errors(m_np, solved_np))
    m, rcond, _weights, _filt = _make(pj, dev, bc, masked=False)
    bias = (bc.m0[0] - _n(m)[0])[bc.src]
    print("unmasked: the source's I is low by", bias, "against the bar %.3g" % bar)
    assert (bias > bar).all()


def test_bins_none_reproduces_todays_output_by_bits(pj, dev, bc):
    """bins=None is filter_bin_map_pol_nearest_tod, which itself makes the calls it made before."""
    mask = pj.Enmap(to_dev(bc.fit_mask, dev), bc.wcs)
    today = pj.filter_bin_map_pol_nearest_tod(*_args(bc, dev), bc.seg_start, 3, fit_mask=mask, rcond_min=BC.RCOND_MIN)
    spelled = pj.template_bin_map_pol_nearest_tod(*_args(bc, dev), None, bc.seg_start, 3, fit_mask=mask, rcond_min=BC.RCOND_MIN)
    comp = pj.polyfilter_tod(to_dev(bc.tod, dev), bc.seg_start, 3, w=to_dev(bc.w_fit(True), dev))
    assert bits_equal(_n(today[3]), _n(comp)) and bits_equal(_n(spelled[3]), _n(comp))
    for a, b in zip(today[:3], spelled[:3]):                                  # map, rcond, weights: sums of the same terms in the atomics' order
        assert np.abs(_n(a) - _n(b)).max() <= 1e-9 * max(1.0, np.abs(_n(a)).max())


def test_polynomial_then_bins_then_modes_is_the_three_calls_by_hand(pj, dev, bc):
    """The filtered timestream by bits, the map to the scatters' clause; tod is not changed; and the run with the bins alone."""
    wf = to_dev(bc.w_fit(True), dev)
    gains = to_dev(np.linspace(0.8, 1.2, BC.ND), dev)
    tod = to_dev(bc.tod, dev)
    all3 = _make(pj, dev, bc, order=1, modes=gains)
    step = pj.polyfilter_tod(tod, bc.seg_start, 1, w=wf)
    step = pj.binfilter_tod(step, _plan(bc, dev), w=wf)
    step = pj.modefilter_tod(step, gains, w=wf)
    assert bits_equal(_n(all3[3]), _n(step)) and bits_equal(_n(tod), bc.tod)
    by_hand = pj.binned_map_pol_nearest_tod(step, to_dev(bc.w, dev), bc.q_bore.to(dev), bc.q_det.to(dev), None, bc.shape, bc.wcs, rcond_min=BC.RCOND_MIN)
    for a, b in zip(all3[:3], by_hand):
        assert np.abs(_n(a) - _n(b)).max() <= 1e-9 * max(1.0, np.abs(_n(a)).max())
    two = _make(pj, dev, bc, modes=gains)                                        # no polynomial step: bins, then modes
    assert bits_equal(_n(two[3]), _n(pj.modefilter_tod(pj.binfilter_tod(tod, _plan(bc, dev), w=wf), gains, w=wf)))
    alone = _make(pj, dev, bc)                                                   # order=None, modes=None, bins=...
    assert bits_equal(_n(alone[3]), _n(pj.binfilter_tod(tod, _plan(bc, dev), w=wf)))


def test_chunked_and_with_one_weight_per_detector(pj, dev, bc):
    whole = _make(pj, dev, bc)
    chunked = _make(pj, dev, bc, chunk_t=100)                                    # chunks that cut sweeps
    assert bits_equal(_n(chunked[3]), _n(whole[3]))
    solved = _n(chunked[1]) >= BC.RCOND_MIN
    assert solved.all() and max(bc.errors(_n(chunked[0]), solved)) <= 1e-10
    per_det = _make(pj, dev, bc, w=bc.w_det)
    assert bits_equal(_n(per_det[3]), _n(whole[3]))
    solved = _n(per_det[1]) >= BC.RCOND_MIN
    assert solved.all() and max(bc.errors(_n(per_det[0]), solved)) <= 1e-10


def test_refusals(pj, dev, bc):
    args = _args(bc, dev)
    order, bin_start = _plan(bc, dev)
    with pytest.raises(ValueError, match="needs modes or bins"):
        pj.template_bin_map_pol_nearest_tod(*args, None)                         # all three filters absent
    with pytest.raises(ValueError, match="filter_bin_map_pol_nearest_tod: order=None skips the polynomial step and needs modes$"):
        pj.filter_bin_map_pol_nearest_tod(*args, None, None)                     # today's refusal, in today's words
    with pytest.raises(TypeError):
        pj.filter_bin_map_pol_nearest_tod(*args, None, None, bins=(order, bin_start))        # that function's arguments are fixed
    with pytest.raises(ValueError, match="one entry per time sample"):
        pj.template_bin_map_pol_nearest_tod(*args, (order[:-1], bin_start))
    with pytest.raises(ValueError, match="one entry per time sample"):
        pj.template_bin_map_pol_nearest_tod(*args, (bc.index[:-1], BC.N_BIN))
    with pytest.raises(ValueError, match="non-decreasing"):
        pj.template_bin_map_pol_nearest_tod(*args, (order, bin_start.flip(0)))
    with pytest.raises(ValueError, match="bins is the"):
        pj.template_bin_map_pol_nearest_tod(*args, order)
    with pytest.raises(TypeError):
        pj.template_bin_map_pol_nearest_tod(*args, (order, bin_start), bc.seg_start, 0, None, 1e-3, 1e-10, None, None)       # modes is keyword-only
