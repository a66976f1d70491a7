"""pj.filter_bin_map_pol_nearest_tod with modes= on the device, on tests/modefilter_case.py: a 24 x 12 patch, 8
detectors in two groups, a zero sky with one compact source, one white common signal per group of 10^3 times the source seen
through per-detector gains, no noise.

The bar of the filtered case is the numpy composition's own error on the case times 4: with m_ld the composition whose filter runs
in long double, |m_numpy - m_ld| worst over the solved pixels; the device's map is held to |m_device - m_ld| <= 4 x that.  (The sky
itself is 6e-14 from m_ld: the filtered timestream is rounded to Float64 before it is binned.)"""
import numpy as np
import pytest
import torch
from gpu_support import dev, to_dev

import modefilter_case as MC
from conftest import bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc(pj, O):
    return MC.Case(pj, O)


def _n(e):
    return e.data.cpu().numpy() if hasattr(e, "data") and not isinstance(e, torch.Tensor) else e.cpu().numpy()


def _args(mc, dev):
    return (to_dev(mc.tod, dev), to_dev(mc.w, dev), mc.q_bore.to(dev), mc.q_det.to(dev), None, mc.shape, mc.wcs)


def _make(pj, dev, mc, with_modes, order=None, chunk_t=None, **kw):
    """With modes: the mask, the gains and the two groups, no polynomial step unless `order` is given.  Without: the polynomial
    step alone, at MC.POLY_ORDER (the map-maker has no run with neither)."""
    mask = pj.Enmap(to_dev(mc.fit_mask, dev), mc.wcs)
    if with_modes:
        kw = dict(dict(modes=to_dev(mc.gains, dev), grp_start=MC.GRP_START), **kw)
    else:
        order = MC.POLY_ORDER
    return pj.filter_bin_map_pol_nearest_tod(*_args(mc, dev), mc.seg_start if order is not None else None, order, fit_mask=mask,
                                             rcond_min=MC.RCOND_MIN, chunk_t=chunk_t, **kw)


def test_with_the_mask_and_the_gains_the_map_is_the_sky(pj, dev, mc):
    """The test that fails without the feature."""
    m_ld, solved_ld, _f = mc.yardstick(True, np.longdouble)
    m_np, solved_np, _f = mc.yardstick(True)
    bar = 4 * max(mc.errors(m_np, solved_np, m_ld))
    m, rcond, _weights, filt = _make(pj, dev, mc, True)
    solved = _n(rcond) >= MC.RCOND_MIN
    on, off = mc.errors(_n(m), solved, m_ld)
    print("filtered: numpy's error against long double %.3g (bar %.3g); device on the source %.3g, off it %.3g; device against the sky %.3g"
          % (bar / 4, bar, on, off, max(mc.errors(_n(m), solved))))
    assert solved.all() and solved_np.all() and solved_ld.all()
    assert on <= bar and off <= bar
    assert max(mc.errors(_n(m), solved)) <= 1e-10                            # and so it is the sky, to the rounding of a 10^3 signal
    # the filtered timestream is modefilter_tod of the timestream with the masked weights, in bits, and tod is not changed
    comp = pj.modefilter_tod(to_dev(mc.tod, dev), to_dev(mc.gains, dev), w=to_dev(mc.w_fit(True), dev), grp_start=MC.GRP_START)
    assert bits_equal(_n(filt), _n(comp))


def test_without_modes_the_map_is_wrong_by_more_than_the_source(pj, dev, mc):
    m, rcond, _weights, _filt = _make(pj, dev, mc, False)
    solved = _n(rcond) >= MC.RCOND_MIN
    worst = max(mc.errors(_n(m), solved))
    print("without modes: worst |map - sky| = %.3g" % worst)
    assert solved.all() and worst > MC.SRC_IQU[0]


def test_modes_none_reproduces_the_polynomial_only_output_by_bits(pj, dev, mc):
    """modes=None, spelled out or left out, with the other two new arguments given or not: the filtered timestream is
    polyfilter_tod's in bits, and the maps of the runs are each other's to the atomics' last bits (the binning is not
    bit-reproducible between any two runs: the scatters' clause)."""
    mask = pj.Enmap(to_dev(mc.fit_mask, dev), mc.wcs)
    today = pj.filter_bin_map_pol_nearest_tod(*_args(mc, dev), mc.seg_start, 3, fit_mask=mask, rcond_min=MC.RCOND_MIN)
    spelled = pj.filter_bin_map_pol_nearest_tod(*_args(mc, dev), mc.seg_start, 3, fit_mask=mask, rcond_min=MC.RCOND_MIN, modes=None,
                                                grp_start=MC.GRP_START, mode_rcond_min=0.5)
    comp = pj.polyfilter_tod(to_dev(mc.tod, dev), mc.seg_start, 3, w=to_dev(mc.w_fit(True), dev))
    assert bits_equal(_n(today[3]), _n(comp)) and bits_equal(_n(spelled[3]), _n(comp))
    for a, b in zip(today[:3], spelled[:3]):                                  # map, rcond, weights: sums of the same terms in the atomics' order
        assert np.abs(_n(a) - _n(b)).max() <= 1e-9 * max(1.0, np.abs(_n(a)).max())


def test_polynomial_first_then_modes_in_place_and_chunked(pj, dev, mc):
    """With an order and modes the filtered timestream is modefilter_tod of polyfilter_tod, the same masked weights in both, by
    bits; a run in chunks that cut sweeps gives the same filtered timestream by bits, with and without the polynomial step."""
    wf = to_dev(mc.w_fit(True), dev)
    both = _make(pj, dev, mc, True, order=1)
    comp = pj.modefilter_tod(pj.polyfilter_tod(to_dev(mc.tod, dev), mc.seg_start, 1, w=wf), to_dev(mc.gains, dev), w=wf, grp_start=MC.GRP_START)
    assert bits_equal(_n(both[3]), _n(comp))
    assert bits_equal(_n(_make(pj, dev, mc, True, order=1, chunk_t=100)[3]), _n(both[3]))
    whole, chunked = _make(pj, dev, mc, True), _make(pj, dev, mc, True, chunk_t=100)
    assert bits_equal(_n(chunked[3]), _n(whole[3]))
    solved = _n(chunked[1]) >= MC.RCOND_MIN
    assert solved.all() and max(mc.errors(_n(chunked[0]), solved)) <= 1e-10


def test_refusals(pj, dev, mc):
    args = _args(mc, dev)
    g = to_dev(mc.gains, dev)
    with pytest.raises(ValueError, match="order=None"):
        pj.filter_bin_map_pol_nearest_tod(*args, None, None)
    with pytest.raises(TypeError):
        pj.filter_bin_map_pol_nearest_tod(*args, mc.seg_start, 0, None, 1e-3, 1e-10, None, g)        # modes is keyword-only
    with pytest.raises(ValueError, match="grp_start must be non-decreasing"):
        pj.filter_bin_map_pol_nearest_tod(*args, None, None, modes=g, grp_start=[0, 5, 4, 8])
    with pytest.raises(ValueError, match=r"inside \[0, D\]"):
        pj.filter_bin_map_pol_nearest_tod(*args, None, None, modes=g, grp_start=[0, 9])
    with pytest.raises(ValueError, match=r"modes is a \(D, K\)"):
        pj.filter_bin_map_pol_nearest_tod(*args, None, None, modes=g[:-1])
    with pytest.raises(ValueError, match="Float64 modes"):
        pj.filter_bin_map_pol_nearest_tod(*args, None, None, modes=g.float())
    with pytest.raises(ValueError, match="rcond_min"):
        pj.filter_bin_map_pol_nearest_tod(*args, None, None, modes=g, mode_rcond_min=1.0)
    with pytest.raises(ValueError, match="non-decreasing"):
        pj.filter_bin_map_pol_nearest_tod(*args, mc.seg_start[::-1], 1, modes=g)
