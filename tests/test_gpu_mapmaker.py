"""pj.cg_map_pol on the device against the CPU yardstick tests/normal_ref.py, on the inputs of
tests/test_mapmaker_ref.py: the sparse direct solve, kappa of the pencil (A, M) and the bars derived there
(|x - x*|_A <= sqrt(kappa) tol |x*|_A; normal_ref.iteration_cap).  The device's right-hand side and operator differ from the
yardstick's by rounding (~kappa * 2^-53 relative in x*), orders below the bar at tol = 1e-8.  fused=True and fused=False are each
held to the yardstick; their results are never compared with each other bit for bit."""
import numpy as np
import pytest

import normal_ref as NR

torch = pytest.importorskip("torch")
from gpu_support import dev, to_dev
pytestmark = pytest.mark.gpu


def _batches(c, d, dev, parts=1):
    cuts = np.linspace(0, len(d), parts + 1).astype(int)
    return [(to_dev(d[a:b], dev), to_dev(c.w[a:b], dev), to_dev(c.sky[a:b], dev), to_dev(c.resp[a:b], dev)) for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("geom", ["box_5x7", "box_24x12", "box_2x2"])
def test_small_shapes_meet_the_yardsticks_bars(pj, O, dev, geom, fused):
    c = NR.case(pj, O, geom)
    tol = 1e-8
    m, rcond, info = pj.cg_map_pol(_batches(c, c.d, dev), c.shape, c.wcs, tol=tol, fused=fused)
    assert isinstance(m, pj.Enmap) and tuple(m.data.shape) == (3, c.shape[1], c.shape[0]) and tuple(rcond.data.shape) == (c.shape[1], c.shape[0])
    xs = c.direct(c.d)
    cap = NR.iteration_cap(c.kappa, tol)
    err, bar = c.anorm(m.data.cpu().numpy().ravel() - xs), np.sqrt(c.kappa) * tol * c.anorm(xs)
    print("%s fused=%s: %d iterations (cap %d), |x - x*|_A / bound = %.3g, min rcond %.3g" % (
        geom, fused, info["iterations"], cap, err / bar, float(rcond.data.min())))
    assert info["converged"] and not info["breakdown"] and len(info["history"]) == info["iterations"]
    assert info["iterations"] <= cap
    assert err <= bar
    assert float(rcond.data.min()) >= NR.RCOND_MIN


def _compose_a(pj, batches, x, shape, wcs):
    y = None
    for _d, w, sky, resp in batches:
        y = pj.scatter_pol(w * pj.sample_pol(x, sky, resp), sky, resp, shape, wcs, out=y)
    return y


def test_full_sky_in_three_batches(pj, O, dev):
    """The (90, 46) map, 2 * 10^5 pixel-uniform points in three batches: converges within the cap, and the TRUE residual
    b - A x, recomputed with the composition scatter_pol(w * sample_pol(x)), meets the stopping rule to 1 %: the recursive and
    the true residual agree to ~10 digits at this conditioning."""
    c = NR.case(pj, O, "cc_90x46")
    tol = 1e-8
    batches = _batches(c, c.d, dev, parts=3)
    m, rcond, info = pj.cg_map_pol(batches, c.shape, c.wcs, tol=tol, fused=True)
    cap = NR.iteration_cap(c.kappa, tol)
    b = weights = None
    for d, w, sky, resp in batches:
        b = pj.scatter_pol(w * d, sky, resp, c.shape, c.wcs, out=b)
        weights = pj.scatter_pol_weights(w, sky, resp, c.shape, c.wcs, out=weights)
    r = pj.Enmap(b.data - _compose_a(pj, batches, m, c.shape, c.wcs).data, c.wcs)
    rz = float(torch.dot(r.data.view(-1), pj.pol_block_solve(r, weights).data.view(-1)))
    rz0 = float(torch.dot(b.data.view(-1), pj.pol_block_solve(b, weights).data.view(-1)))
    rel = np.sqrt(rz / rz0)
    print("full sky: kappa = %.3g, %d iterations (cap %d), true residual %.3g, recursive %.3g" % (c.kappa, info["iterations"], cap, rel, info["history"][-1]))
    assert info["converged"] and info["iterations"] <= cap
    assert rel <= 1.01 * tol
    assert bool((rcond.data >= NR.RCOND_MIN).all())


def test_noiseless_samples_recover_the_sky_and_the_binned_map_does_not(pj, O, dev):
    c = NR.case(pj, O, "box_80x40")
    top = float(np.abs(c.m0).max())
    batches = _batches(c, c.d0, dev)
    m, _rcond, info = pj.cg_map_pol(batches, c.shape, c.wcs, tol=1e-10, fused=True)
    binned, _rc = pj.binned_map_pol(*batches[0], c.shape, c.wcs)
    cg = float(np.abs(m.data.cpu().numpy() - c.m0).max())
    off = float(np.abs(binned.data.cpu().numpy() - c.m0).max())
    print("noiseless: max|x - m0| = %.3g after %d iterations, binned map off by %.3g, max|m0| = %.3g" % (cg, info["iterations"], off, top))
    assert info["converged"]
    assert cg <= 1e-6 * top
    assert off > 0.1 * top


@pytest.mark.parametrize("fused", [True, False])
def test_masked_pixels_stay_zero(pj, O, dev, fused):
    c = NR.case(pj, O, "cc_90x46", masked=True)
    tol = 1e-8
    m, rcond, info = pj.cg_map_pol(_batches(c, c.d, dev, parts=2), c.shape, c.wcs, tol=tol, fused=fused)
    x, rc = m.data.cpu().numpy(), rcond.data.cpu().numpy()
    cap = NR.iteration_cap(c.kappa, tol)
    print("masked fused=%s: %d iterations (cap %d)" % (fused, info["iterations"], cap))
    assert info["converged"] and info["iterations"] <= cap
    for rows in (slice(0, 8), slice(37, 46)):
        assert not x[:, rows].view(np.int64).any(), "an unhit pixel is not +0.0 as bits"
        assert not rc[rows].view(np.int64).any(), "an unhit pixel's rcond is not +0.0 as bits"
    solved = c.solved.reshape(c.shape[1], c.shape[0])
    assert np.array_equal(rc >= NR.RCOND_MIN, solved) and (x[:, solved] != 0).all()
    xs = c.direct(c.d)
    assert c.anorm(x.ravel() - xs) <= np.sqrt(c.kappa) * tol * c.anorm(xs)


def test_maxiter_and_nan_samples(pj, O, dev):
    c = NR.case(pj, O, "box_24x12")
    batches = _batches(c, c.d, dev)
    m, _rcond, info = pj.cg_map_pol(batches, c.shape, c.wcs, maxiter=2, fused=True)
    assert not info["converged"] and not info["breakdown"] and info["iterations"] == 2 and len(info["history"]) == 2
    assert bool(torch.isfinite(m.data).all()) and float(m.data.abs().max()) > 0
    d = c.d.copy()
    d[1234] = np.nan
    for fused in (True, False):
        with pytest.raises(ValueError, match="finite"):
            pj.cg_map_pol(_batches(c, d, dev), c.shape, c.wcs, fused=fused)
    with pytest.raises(ValueError):
        pj.cg_map_pol([], c.shape, c.wcs)
    with pytest.raises(ValueError, match="rcond_min"):
        pj.cg_map_pol(batches, c.shape, c.wcs, rcond_min=0.0)
