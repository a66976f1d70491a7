"""pj.ml_map_pol_nearest_tod on the device, on tests/ml_map_case.py: a 16 x 10 patch, 4 detectors, 3000 samples in
three crossing scans, 10 % cuts with NaN under them, a kernel of lambda = 64 from a 1 / f spectrum.

THE BAR.  pcg stops when the M^-1 norm of the residual has fallen by `tol`; the error of the map is then at most about
cond(M^-1/2 A M^-1/2) tol of the map, so the device must agree with the dense numpy solution (toeplitz_ref.MLSystem, which
tests/test_toeplitz_ref.py runs without a device) within 10 tol cond max|m|, the condition number computed on the CPU from the
dense system.  Rounding, and the order of the scatters' atomics, are orders of magnitude below that at tol = 1e-8."""
import numpy as np
import pytest
import torch
from gpu_support import dev, to_dev

import ml_map_case as MC
import nearest_ref
from conftest import bits_equal

pytestmark = pytest.mark.gpu

TOL = 1e-8
CHUNKS = (None, 700, 1303)                                      # one chunk; chunks that cut the scans of 1000 and do not divide T = 3000


@pytest.fixture(scope="module")
def ml(pj, O):
    return MC.case(pj, O)


def _make(pj, dev, ml, tod, chunk_t=None, kernel=None, w=None, **kw):
    kernel = ml.kernel if kernel is None else kernel
    m, rcond, weights, info = pj.ml_map_pol_nearest_tod(to_dev(tod, dev), to_dev(ml.w if w is None else w, dev), ml.q_bore.to(dev), ml.q_det.to(dev),
                                                        None, ml.shape, ml.wcs, to_dev(kernel, dev), ml.seg_start, rcond_min=MC.RCOND_MIN, tol=TOL,
                                                        chunk_t=chunk_t, **kw)
    return m.data.cpu().numpy(), rcond.data.cpu().numpy(), weights.data.cpu().numpy(), info


@pytest.mark.parametrize("seed", [None, MC.SEEDS[0]], ids=["noiseless", "noisy"])
def test_it_is_the_dense_solution_in_any_chunks(pj, dev, ml, seed):
    """Without noise the solution is the sky itself; with 1 / f noise it is the dense solve's map.  The timestream is NaN under every
    cut.  The same bar holds in chunks that cut the scans, so the chunkings agree with each other to twice it."""
    s = ml.system()
    tod = ml.tod(seed)
    want = s.solve(tod)
    bar = 10 * TOL * s.pcond * float(np.abs(want).max())
    for chunk_t in CHUNKS:
        m, rcond, weights, info = _make(pj, dev, ml, tod, chunk_t)
        err = float(np.abs(m - want).max())
        print("%s, chunk_t %s: %d iterations, |map - dense| %.3g, bar %.3g (cond %.3g)" % (
            "noiseless" if seed is None else "noisy", chunk_t, info["iterations"], err, bar, s.pcond))
        assert info["converged"] and not info["breakdown"]
        assert (rcond >= MC.RCOND_MIN).all() and np.allclose(rcond, s.rcond, rtol=1e-9) and np.allclose(weights, s.w6, rtol=1e-9)
        assert err <= bar
        if seed is None:
            assert float(np.abs(m - ml.m0).max()) <= bar                    # noiseless samples recover the sky on the solved pixels


def test_lambda_zero_is_the_binned_map_after_one_update(pj, dev, ml):
    """With lambda = 0 and kernel = w_det the system is exactly its pixel blocks: pcg ends within 2 iterations on
    binned_map_pol_nearest_tod's map for the weights w_det [w > 0]."""
    w_det = 10.0 ** np.random.default_rng(3).uniform(-0.5, 0.5, MC.ND)
    tod = ml.tod(MC.SEEDS[1])
    m, _rcond, _weights, info = _make(pj, dev, ml, tod, 1303, kernel=w_det[:, None])
    finite = np.where(ml.w > 0, tod, 0.0)
    mb, _rb, _wb = pj.binned_map_pol_nearest_tod(to_dev(finite, dev), to_dev(w_det[:, None] * ml.w, dev), ml.q_bore.to(dev), ml.q_det.to(dev), None,
                                                 ml.shape, ml.wcs, rcond_min=MC.RCOND_MIN)
    mb = mb.data.cpu().numpy()
    print("lambda 0: %d iterations, |ML - binned| %.3g" % (info["iterations"], np.abs(m - mb).max()))
    assert info["converged"] and info["iterations"] <= 2
    assert np.abs(m - mb).max() <= 10 * TOL * np.abs(mb).max()


def test_an_unsolved_pixel_stays_zero_and_its_sample_is_never_read(pj, O, dev, ml):
    """All samples of one pixel but one are cut: a single hit, the pixel is unsolved and stays +0.0 in all three planes.  Its one
    sample is live in w, so only g cuts it: setting it to 1e6 must not change any other pixel BY BITS.  Two runs can be compared by
    bits only where the order of the scatters' atomic adds is fixed, so this test runs in chunks of 16 time samples: the 64 samples
    of a chunk are one wavefront's, and successive launches are ordered by the stream."""
    idx = nearest_ref.taps(O, ml.wcs, ml.shape, ml.sky)[0].reshape(MC.ND, MC.NT)
    det, t = 0, 1234
    assert ml.w[det, t] > 0
    pix = idx[det, t]
    w = ml.w.copy()
    w[idx == pix] = 0.0
    w[det, t] = 1.0
    tod = ml.tod(MC.SEEDS[2])
    tod[(w == 0) & ~np.isnan(tod)] = np.nan
    loud = tod.copy()
    loud[det, t] = 1e6
    a, b = (_make(pj, dev, ml, d, 16, w=w) for d in (tod, loud))
    nx = ml.shape[0]
    py, px = divmod(int(pix), nx)
    assert a[1][py, px] < MC.RCOND_MIN and (np.delete(a[1].ravel(), pix) >= MC.RCOND_MIN).all()
    for m, _rcond, _weights, info in (a, b):
        assert info["converged"]
        assert bits_equal(m[:, py, px], np.zeros(3))
    assert bits_equal(a[0], b[0]), "a sample on an unsolved pixel reached the map"
    err = np.abs(np.delete((a[0] - ml.m0).reshape(3, -1), pix, axis=1))
    assert err.max() < 5 * MC.SIGMA                                            # the rest of the map is still a map of the sky


def test_refusals(pj, dev, ml):
    args = (to_dev(np.where(ml.w > 0, ml.tod(), 0.0), dev), to_dev(ml.w, dev), ml.q_bore.to(dev), ml.q_det.to(dev), None, ml.shape, ml.wcs)
    k = to_dev(ml.kernel, dev)
    with pytest.raises(ValueError, match="kernel is a"):
        pj.ml_map_pol_nearest_tod(*args, k[:3], ml.seg_start)
    with pytest.raises(ValueError, match="c_0"):
        pj.ml_map_pol_nearest_tod(*args, -k, ml.seg_start)
    with pytest.raises(ValueError, match="non-decreasing"):
        pj.ml_map_pol_nearest_tod(*args, k, ml.seg_start[::-1])
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        pj.ml_map_pol_nearest_tod(*args, k.cpu(), ml.seg_start)
