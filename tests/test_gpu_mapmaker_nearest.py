"""The map of nearest-pixel pointing on the device: pj.binned_map_pol_nearest, and the fact it rests on -- with one
pixel per point P^T W P is exactly the pixel blocks scatter_pol_weights_nearest accumulates.

Inputs are nearest_ref.map_case's: noiseless samples d = P m0 of a random sky, at least 48 points per pixel on average, random psi,
w = 10^U(-1, 1), three batches, three pixels without a hit.  tests/test_nearest_ref.py holds the numpy recipe to the same bounds
on the same inputs."""
import numpy as np
import pytest

import nearest_ref as N
import scatter_ref as R

torch = pytest.importorskip("torch")
from gpu_support import bits, dev, to_dev
pytestmark = pytest.mark.gpu

MAP_GEOMS = ("box_5x7", "box_80x40", "cc_360x181")


_dev_cases = {}


def _device_case(pj, O, dev, geom):
    """The case's arrays on the device, once per geometry: (case, [(d, w, sky, resp) per batch], (d, w, sky, resp) whole)."""
    if geom not in _dev_cases:
        c = N.map_case(pj, O, geom)
        whole = (to_dev(c.d, dev), to_dev(c.w, dev), to_dev(c.sky, dev), to_dev(c.resp, dev))
        _dev_cases[geom] = (c, [tuple(t[s] for t in whole) for s in c.batches], whole)
    return _dev_cases[geom]


# ---- 8. the map -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("geom", MAP_GEOMS)
def test_the_map_recovers_the_sky(pj, O, dev, geom, fused):
    """binned_map_pol_nearest of noiseless d = P m0 in three batches returns m0 on every solved pixel within
    16 (k + 50) 2^-52 ||m0(p)||_1 / rc(p) (nearest_ref.map_bound: the pixel's own triple, term count and rcond); unhit pixels are
    +0.0 as bits in the map and in rcond; the returned weights are what bin_pol_nearest accumulates when called separately."""
    c, batches, _whole = _device_case(pj, O, dev, geom)
    m, rc, wts = pj.binned_map_pol_nearest(batches, c.shape, c.wcs, fused=fused)
    assert all(isinstance(e, pj.Enmap) for e in (m, rc, wts))
    nx, ny = c.shape
    assert tuple(m.data.shape) == (3, ny, nx) and tuple(rc.data.shape) == (ny, nx) and tuple(wts.data.shape) == (6, ny, nx)
    m, rc, wts = m.data.cpu().numpy(), rc.data.cpu().numpy(), wts.data.cpu().numpy()
    solved = rc >= N.RCOND_MIN
    assert np.array_equal(solved, c.solved), "%d pixels solved on one side only" % int((solved != c.solved).sum())
    assert solved[c.hits > 0].mean() >= (0.95 if geom == "cc_360x181" else 1.0)
    err = np.abs(m - c.m0).max(axis=0)
    b = N.map_bound(c.m0, c.hits, rc)
    print("%s, %s: worst error / bound = %.3g on %d solved pixels, worst error %.3g, min rcond %.3g" % (
        geom, "fused" if fused else "composed", float((err[solved] / b[solved]).max()), int(solved.sum()), float(err[solved].max()),
        float(rc[solved].min())))
    assert np.all(err[solved] <= b[solved])
    unhit = c.hits == 0
    assert unhit.sum() == 3
    assert not bits(m[:, ~solved]).any() and not bits(rc[unhit]).any() and not bits(wts[:, unhit]).any()
    # the weights against a separate accumulation, and against the yardstick
    w2 = None
    for d, w, sky, resp in batches:
        _r, w2 = pj.bin_pol_nearest(d, w, sky, resp, c.shape, c.wcs, weights=w2)
    w2 = w2.data.cpu().numpy()
    _rhs_t, (wref, wk, wS) = N.bin(O, c.wcs, c.shape, c.sky, c.resp, c.d, c.w)
    single = c.nz_w <= 1
    assert single.sum() >= 18 and np.array_equal(bits(wts[single]), bits(w2[single])) and np.array_equal(bits(wts[single]), bits(wref[single]))
    R.held(wts, w2, wk, wS, geom + ": returned weights against a separate bin_pol_nearest")
    R.held(wts, wref, wk, wS, geom + ": returned weights against the yardstick")


@pytest.mark.parametrize("geom", MAP_GEOMS)
def test_the_bilinear_binned_map_does_not(pj, O, dev, geom):
    """The contrast the order exists for: pj.binned_map_pol (order 1) of the same samples misses m0 by more than 0.1."""
    c, _batches, (d, w, sky, resp) = _device_case(pj, O, dev, geom)
    m1, rc1 = pj.binned_map_pol(d, w, sky, resp, c.shape, c.wcs)
    m1, rc1 = m1.data.cpu().numpy(), rc1.data.cpu().numpy()
    miss = float(np.abs(m1 - c.m0).max(axis=0)[rc1 >= N.RCOND_MIN].max())
    print("%s: the order-1 binned map misses m0 by %.3g" % (geom, miss))
    assert miss > 0.1


def test_a_non_finite_right_hand_side_raises(pj, O, dev):
    c, batches, _whole = _device_case(pj, O, dev, "box_5x7")
    d, w, sky, resp = batches[1]
    bad = d.clone()
    bad[7] = float("inf")
    for fused in (True, False):
        with pytest.raises(ValueError, match="not finite"):
            pj.binned_map_pol_nearest([batches[0], (bad, w, sky, resp)], c.shape, c.wcs, fused=fused)


# ---- 9. P^T W P is the blocks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", MAP_GEOMS)
def test_the_normal_operator_is_the_blocks(pj, O, dev, geom):
    """scatter_pol_nearest(w * sample_pol_nearest(x)) against pol_block_apply(x, weights) per pixel within nearest_ref.blocks_bound
    (derived there: the composition's (k, S) plus the roundings of the block product), and pj.pcg with these two operators
    converges in at most 2 iterations at tol = 1e-8."""
    c, _batches, (d, w, sky, resp) = _device_case(pj, O, dev, geom)
    x = np.random.default_rng(5).normal(size=c.m0.shape)
    wts = pj.scatter_pol_weights_nearest(w, sky, resp, c.shape, c.wcs)

    def apply_a(p):
        return pj.scatter_pol_nearest(w * pj.sample_pol_nearest(pj.Enmap(p, c.wcs), sky, resp), sky, resp, c.shape, c.wcs).data

    def apply_minv(r):
        return pj.pol_block_solve(pj.Enmap(r, c.wcs), wts, rcond_min=N.RCOND_MIN).data

    comp = apply_a(to_dev(x, dev)).cpu().numpy()
    blk = pj.pol_block_apply(pj.Enmap(to_dev(x, dev), c.wcs), wts).data.cpu().numpy()
    b = N.blocks_bound(O, c.wcs, c.shape, x, c.sky, c.resp, c.w)
    gap = np.abs(comp - blk)
    print("%s: composition against the blocks, worst gap / bound = %.3g" % (geom, float((gap[b > 0] / b[b > 0]).max())))
    assert np.all(gap <= b) and (b[:, c.hits > 0] > 0).all()
    rhs = pj.scatter_pol_nearest(w * d, sky, resp, c.shape, c.wcs).data
    sol, info = pj.pcg(apply_a, apply_minv, rhs, 1e-8, 10)
    print("%s: pcg took %d iterations, history %s" % (geom, info["iterations"], info["history"]))
    assert info["converged"] and not info["breakdown"] and 1 <= info["iterations"] <= 2
    sol = sol.cpu().numpy()
    assert float(np.abs(sol - c.m0).max(axis=0)[c.solved].max()) < 1e-10 and not bits(sol[:, ~c.solved]).any()


# ---- 10. exact sums: the four paths by bits -------------------------------------------------------------------------------------------
def test_exact_sums_do_not_depend_on_the_path(pj, O, dev):
    """With integer inputs every term and every partial sum of a pixel is a small integer (the largest sum is 52, the largest sum
    of |terms| 98), exact in Float64 in whatever order the atomic adds arrive, so the paths of binned_map_pol_nearest can be held
    to each other and to the yardstick by bits: one batch or three (1, 64 and 257 points), fused or composed.  box_5x7 with
    nearest_ref.points' 322 positions (pixel-edge ties, off-map points, three non-finite positions: 152 on the map, all 35 pixels
    hit), d integers in [-8, 8], w in {1, 2, 4}, responses in {-1, 0, 1}.  weights: np.add.at of the nine integer terms at
    nearest_ref.cells' pixels; rcond and the map: polsolve_ref.solve of those sums, whose bits the device is to give.  The solved
    set is the yardstick's (25 pixels at rcond_min = 1e-3) and at least half of the hit pixels: a condition on the input."""
    import pol_ref
    import polsolve_ref
    shape, wcs = N.geometries(pj)["box_5x7"]
    nx, ny = shape
    n = 322
    sky = N.points(O, wcs, shape, n, seed=0)
    rng = np.random.default_rng(100)
    d = rng.integers(-8, 9, n).astype(np.float64)
    w = 2.0 ** rng.integers(0, 3, n)
    resp = rng.integers(-1, 2, (n, 2)).astype(np.float64)
    idx = N.cells(O, wcs, shape, sky)[0]
    on = idx >= 0
    rhs, w6 = np.zeros((3, ny * nx)), np.zeros((6, ny * nx))
    for ref, t in ((rhs, pol_ref.terms(w * d, resp, 0)), (w6, pol_ref.terms(w, resp, 1))):
        for c in range(len(ref)):
            np.add.at(ref[c], idx[on], t[c][on])
    hit = np.bincount(idx[on], minlength=ny * nx) > 0
    x, rc, info = polsolve_ref.solve(w6, rhs, N.RCOND_MIN)
    print("%d of %d points on the map, %d pixels hit, %d solved, largest sum %g" % (on.sum(), n, hit.sum(), info["ok"].sum(), max(np.abs(rhs).max(), w6.max())))
    assert hit.all() and 2 * info["ok"].sum() >= hit.sum()
    whole = (to_dev(d, dev), to_dev(w, dev), to_dev(sky, dev), to_dev(resp, dev))
    batches = [tuple(t[a:b] for t in whole) for a, b in ((0, 1), (1, 65), (65, n))]
    for what, given, fused in (("one batch, fused", [whole], True), ("one batch, composed", [whole], False),
                               ("three batches, fused", batches, True), ("three batches, composed", batches, False)):
        m, rcond, wts = (e.data.cpu().numpy() for e in pj.binned_map_pol_nearest(given, shape, wcs, rcond_min=N.RCOND_MIN, fused=fused))
        assert np.array_equal(bits(wts), bits(w6.reshape(6, ny, nx))), what
        assert np.array_equal(bits(rcond), bits(rc.reshape(ny, nx))), what
        assert np.array_equal(bits(m), bits(x.reshape(3, ny, nx))), what
        assert np.array_equal(rcond >= N.RCOND_MIN, info["ok"].reshape(ny, nx)), what
