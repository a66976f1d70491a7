"""pj.filter_bin_map_pol_nearest_tod on the device, on tests/filter_bin_case.py: a 24 x 12 patch, 4 detectors, a
raster of 24 sweeps with one segment per sweep, a zero sky with one compact source, a random cubic of 10^3 times the source on every
(detector, sweep), no noise.

The bar of the masked case is the CPU yardstick's own error on the case (polyfilter_ref + nearest_ref + polsolve_ref, which
tests/test_polyfilter_ref.py runs without a device) times 4: the worst |map - sky| over the solved pixels."""
import numpy as np
import pytest
import torch
from gpu_support import dev, to_dev

import filter_bin_case as FB
import nearest_ref
from conftest import bits_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fb(pj, O):
    return FB.Case(pj, O)


def _make(pj, dev, fb, masked, chunk_t=None, w=None):
    mask = pj.Enmap(to_dev(fb.fit_mask, dev), fb.wcs) if masked else None
    return pj.filter_bin_map_pol_nearest_tod(to_dev(fb.tod, dev), to_dev(fb.w if w is None else w, dev), fb.q_bore.to(dev), fb.q_det.to(dev), None, fb.shape,
                                             fb.wcs, fb.seg_start, FB.ORDER, fit_mask=mask, rcond_min=FB.RCOND_MIN, chunk_t=chunk_t)


def _sym(p6):
    """(3, 3, ny, nx) from the six planes II, IQ, IU, QQ, QU, UU."""
    ii, iq, iu, qq, qu, uu = p6
    return np.array([[ii, iq, iu], [iq, qq, qu], [iu, qu, uu]])


def _same_map(O, fb, filt, a, b):
    """Two binned maps (map, weights) of one filtered timestream, each the block solve of its own atomic accumulation of the same
    terms, compared without an inverse: A (m_a - m_b) = (r_a - r_b) - (A_a - A_b) m_b up to the two solves' backward errors.  Per
    plane c and pixel, with k terms, S_c = sum|rhs term| and Sabs_cj = sum|weight term| from the yardstick: two accumulations
    differ by k 2^-52 S under the scatters' clause (tests/test_gpu_pointing.py's form), so
    |A dm|_c <= k 2^-52 (S_c + sum_j Sabs_cj |m_j|) + 32 eps sum_j |A_cj| |m_j|, the last term 16 eps |A||m| per 3 x 3 solve."""
    (_rhs, k, S), (_w6, _k6, S6) = nearest_ref.bin(O, fb.wcs, fb.shape, fb.sky, fb.resp, filt.reshape(-1), fb.w.reshape(-1))
    (ma, wa), (mb, _wb) = a, b
    A, Sabs, am = _sym(wa), _sym(S6), np.abs(mb)
    lhs = np.abs(np.einsum("cjyx,jyx->cyx", A, ma - mb))
    eps = 2.0 ** -52
    bound = k * eps * (S + np.einsum("cjyx,jyx->cyx", Sabs, am)) + 32 * eps * np.einsum("cjyx,jyx->cyx", np.abs(A), am)
    return bool((lhs <= bound).all()), float((lhs / np.where(bound > 0, bound, 1.0)).max())


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
def test_it_is_the_composition(pj, O, dev, fb, masked):
    """filtered_tod is polyfilter_tod(tod, seg_start, order, w=w_fit) in bits, w_fit built on the host from the numpy pointing;
    the map is binned_map_pol_nearest_tod of it to the scatters' rounding clause (_same_map).  In chunks that cut sweeps the
    filtered timestream keeps its bits, and so it does with one weight per detector."""
    n = lambda e: e.data.cpu().numpy() if hasattr(e, "data") and not isinstance(e, torch.Tensor) else e.cpu().numpy()
    m, rcond, weights, filt = _make(pj, dev, fb, masked)
    comp = pj.polyfilter_tod(to_dev(fb.tod, dev), fb.seg_start, FB.ORDER, w=to_dev(fb.w_fit(masked), dev))
    assert bits_equal(n(filt), n(comp))
    m2, rcond2, weights2 = pj.binned_map_pol_nearest_tod(comp, to_dev(fb.w, dev), fb.q_bore.to(dev), fb.q_det.to(dev), None, fb.shape, fb.wcs,
                                                         rcond_min=FB.RCOND_MIN)
    assert (n(rcond) >= FB.RCOND_MIN).all() and (n(rcond2) >= FB.RCOND_MIN).all()
    ok, worst = _same_map(O, fb, n(filt), (n(m), n(weights)), (n(m2), n(weights2)))
    print("composition: worst |A dm| / bound = %.3g" % worst)
    assert ok
    m3, _r3, w3, filt3 = _make(pj, dev, fb, masked, chunk_t=100)
    assert bits_equal(n(filt3), n(filt)) and _same_map(O, fb, n(filt), (n(m3), n(w3)), (n(m), n(weights)))[0]
    _m4, _r4, _w4, filt4 = _make(pj, dev, fb, masked, w=fb.w_det)
    assert bits_equal(n(filt4), n(filt))


def test_masked_it_recovers_the_source_and_the_empty_sky(pj, dev, fb):
    m_ref, solved_ref, filt_ref = fb.yardstick(True)
    bar = 4 * max(fb.errors(m_ref, solved_ref))
    m, rcond, _weights, filt = _make(pj, dev, fb, True)
    solved = rcond.data.cpu().numpy() >= FB.RCOND_MIN
    on, off = fb.errors(m.data.cpu().numpy(), solved)
    print("masked: yardstick's error %.3g (bar %.3g); device on the source %.3g, off it %.3g" % (bar / 4, bar, on, off))
    assert solved.all() and solved_ref.all()
    assert on <= bar and off <= bar


def test_unmasked_the_source_is_biased(pj, dev, fb):
    """First on the yardstick, then on the device: without the mask every source pixel's I is low by more than 10 %."""
    m_ref, _solved, _filt = fb.yardstick(False)
    assert ((fb.m0[0] - m_ref[0])[fb.src] > 0.10 * FB.SRC_IQU[0]).all()
    m = _make(pj, dev, fb, False)[0].data.cpu().numpy()
    bias = (fb.m0[0] - m[0])[fb.src] / FB.SRC_IQU[0]
    print("unmasked: the source's I is low by", bias)
    assert (bias > 0.10).all()


def test_refusals(pj, dev, fb):
    args = (to_dev(fb.tod, dev), to_dev(fb.w, dev), fb.q_bore.to(dev), fb.q_det.to(dev), None, fb.shape, fb.wcs)
    with pytest.raises(ValueError, match="fit_mask is one"):
        pj.filter_bin_map_pol_nearest_tod(*args, fb.seg_start, FB.ORDER, fit_mask=to_dev(fb.fit_mask[:-1], dev))
    with pytest.raises(ValueError, match="non-decreasing"):
        pj.filter_bin_map_pol_nearest_tod(*args, fb.seg_start[::-1], FB.ORDER)
    with pytest.raises(ValueError, match="Float64"):
        pj.filter_bin_map_pol_nearest_tod(*args, fb.seg_start, FB.ORDER, fit_mask=to_dev(fb.fit_mask, dev).float())
