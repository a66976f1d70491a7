"""The second grid-stride trip of the pointing, destriping and block-solve kernels.  stream_grid() caps a streaming launch at 2^20
blocks of 256 lanes (CAP = 2^28 work items); a call with more work sends its first blocks round again with
`k0 += gridDim.x * chunk`, chunk = 256 times the kernel's own points per lane U.  The second trip therefore starts at point U * CAP,
and every call here is just past it.  Float64 throughout.  Three techniques keep that affordable:

  1. per point / per pixel   test_gpu_launch_paths.py's method: a block of L = 1 000 003 inputs is held to the module's own yardstick
                             under that module's own rule, then tiled to n; every element of the big call must have the block's
                             bits (compared as integers: a NaN result is the same NaN in either trip).
  2. transposes              the kernels add with atomics and cut a point whose position is not finite.  n = U * CAP + T points,
                             T = 100 003; the second trip [U CAP, n), the T points before it and T more drawn from the rest of
                             the first trip are live with random inputs, every other point is (NaN, NaN) with NaN value, weight and
                             sample.  The map is held to the numpy yardstick of the live points alone by the module's own
                             clause.  Before the device runs, the CPU shows that the comparison can see the trip: the second trip
                             holds exactly T live points, they reach at least half of the pixels with a non-zero term, and the
                             yardstick without them, or with them counted twice, breaks the clause on at least 90 % of the pixels
                             they touch.
  3. k_baseline_project      a segment is (detector, baseline): 2^19 + 3 or 2^21 + 3 detectors on a chunk of 40 or 10 samples pass
                             the cap with 2.1e7 samples, and every baseline is compared with the yardstick's bits on exact inputs.

Each docstring states n, the number of blocks that take a second trip, and the technique."""
import numpy as np
import pytest

import destripe_ref as DR
import nearest_ref as N
import normal_ref as NR
import pol_ref as P
import polsolve_ref as Q
import scatter_cubic_ref as T3
import scatter_ref as R
import spline_ref as SR
from conftest import DEG, bits_equal
from test_gpu_launch_paths import CAP, L, assert_tiled, first_bad, tiled

torch = pytest.importorskip("torch")
from gpu_support import dev, edge_points, same_bits, to_dev
pytestmark = pytest.mark.gpu

T = 100_003                          # live points of a transpose test's second trip: prime and odd
NAN = float("nan")
SENTINEL = np.array([0x7ff8dead0000beef], dtype=np.uint64).view(np.float64)[0]        # a NaN with a payload


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    torch.cuda.empty_cache()


def _fullsky(pj):
    shape, wcs = pj.fullsky_geometry(1.0 * DEG)
    assert tuple(shape) == (360, 181)
    return shape, wcs


def _bits(t):
    return t.view(torch.int64)


def second_trip_blocks(items, per_block=256):
    """How many blocks of the capped grid go round again for `items` work items (groups of lanes for k_baseline_project)."""
    blocks = -(-items // per_block)
    assert blocks > 1 << 20, "the call does not pass stream_grid's cap"
    return blocks - (1 << 20)


# ================================================================================================
# 1. per-point and per-pixel kernels: a checked block, tiled
# ================================================================================================

def _forward_points(O, wcs, shape, seed):
    """L points as gpu_support.edge_points draws them for the forward kernels (sphere, a 1.5-pixel margin, pixel edges and centres, the
    seam column, the pole rows, far outside) with its six positions that are not finite."""
    sky = edge_points(O, wcs, shape, L, seed, False)
    sky[-6:] = [[np.nan, 0.1], [0.1, np.nan], [np.inf, 0.0], [0.0, -np.inf], [np.nan, np.nan], [-np.inf, np.inf]]
    return sky


def _forward_resp(seed):
    resp = np.random.default_rng(seed).normal(size=(L, 2))
    resp[100] = [np.nan, 1.0]; resp[101] = [0.5, np.nan]; resp[102] = [np.inf, -0.0]; resp[103] = [0.0, 0.0]
    return resp


def _cubic_held(got, c, m, O, wcs, shape, sky, what):
    """The scalar order-3 samples of coefficients c = prefilter(m) against spline_ref's evaluation at the oracle's positions
    (pol_ref.sample_planes): NaN exactly where the position is not finite, spline_ref.bound(m) elsewhere."""
    ref = P.sample_planes(O, wcs, shape, c, sky, order=3, prefiltered=True)
    fin = ~np.isnan(ref[0])
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and (~fin).sum() == 6
    r = SR.worst_ratio(got[:, fin], ref[:, fin], m)
    print("%s: worst error / bound = %.3g over %d points" % (what, r, int(fin.sum())))
    assert r <= 1.0, what
    assert (got[:, fin] != 0).mean() > 0.5


def test_sample_cubic_second_trip(pj, O, dev):
    """pj.sample(order=3, prefiltered=True) -> k_sample_cubic, one point per lane: n = 2^28 + L = 269 435 459 points is 1 052 483
    blocks of 256, so blocks 0 .. 3906 (3907 of them) take a second trip (k0 += 2^28).  Technique 1: the block's samples are held
    to spline_ref's bound against its evaluation of the same coefficients; the big call must tile the block's bits."""
    shape, wcs = _fullsky(pj)
    m = SR.input_map("normal", shape, seed=41, nc=1)
    c = SR.prefilter(m, True)
    sky = _forward_points(O, wcs, shape, 42)
    em, d_blk = pj.Enmap(to_dev(c, dev), wcs), to_dev(sky, dev)
    r_blk = pj.sample(em, d_blk, order=3, prefiltered=True)
    assert tuple(r_blk.shape) == (1, L)
    _cubic_held(r_blk.cpu().numpy(), c, m, O, wcs, shape, sky, "sample order 3, the block")
    n = CAP + L
    assert second_trip_blocks(n) == 3907
    big = tiled(d_blk, n)
    out = pj.sample(em, big, order=3, prefiltered=True)
    assert tuple(out.shape) == (1, n)
    assert_tiled(_bits(out[0]), _bits(r_blk[0]), "sample order 3")
    del out, big


def test_sample_pol_cubic_second_trip(pj, O, dev):
    """pj.sample_pol(order=3, prefiltered=True) -> k_sample_pol_cubic, one point per lane: n = 2^28 + L points, 3907 blocks take
    a second trip.  Technique 1: the block is test_gpu_pol.py's rule, the bits of (s_I + q s_Q) + u s_U formed in numpy
    (pol_ref.combine) from the device's scalar samples, themselves held to spline_ref's bound; the big call tiles the block."""
    shape, wcs = _fullsky(pj)
    m = SR.input_map("normal", shape, seed=43, nc=3)
    c = SR.prefilter(m, True)
    sky, resp = _forward_points(O, wcs, shape, 44), _forward_resp(45)
    em, d_blk, d_resp = pj.Enmap(to_dev(c, dev), wcs), to_dev(sky, dev), to_dev(resp, dev)
    s = pj.sample(em, d_blk, order=3, prefiltered=True).cpu().numpy()
    _cubic_held(s, c, m, O, wcs, shape, sky, "sample_pol order 3, the block's scalar samples")
    r_blk = pj.sample_pol(em, d_blk, d_resp, order=3, prefiltered=True)
    with np.errstate(invalid="ignore", over="ignore"):
        same_bits(r_blk.cpu().numpy(), P.combine(s, resp), "sample_pol order 3, the block")
    n = CAP + L
    assert second_trip_blocks(n) == 3907
    big_sky, big_resp = tiled(d_blk, n), tiled(d_resp, n)
    out = pj.sample_pol(em, big_sky, big_resp, order=3, prefiltered=True)
    assert_tiled(_bits(out), _bits(r_blk), "sample_pol order 3")
    del out, big_sky, big_resp


def test_sample_pol_bilinear_second_trip(pj, O, dev):
    """pj.sample_pol(order=1) -> k_sample_pol_bilinear, PXL_PSUNR = 2 points per lane: n = 2^29 + L = 537 870 915 points is
    2^28 + 500 002 work items, so 1954 blocks take a second trip (k0 += 2^29).  Technique 1: the block is the bits of pol_ref.sample
    (the oracle's bilinear sampler and the combination in numpy), NaN by position; the big call tiles the block."""
    shape, wcs = _fullsky(pj)
    m = np.random.default_rng(46).normal(size=(3, shape[1], shape[0]))
    sky, resp = _forward_points(O, wcs, shape, 47), _forward_resp(48)
    em, d_blk, d_resp = pj.Enmap(to_dev(m, dev), wcs), to_dev(sky, dev), to_dev(resp, dev)
    r_blk = pj.sample_pol(em, d_blk, d_resp)
    with np.errstate(invalid="ignore", over="ignore"):
        want = P.sample(O, wcs, shape, m, sky, resp)
    same_bits(r_blk.cpu().numpy(), want, "sample_pol order 1, the block")
    assert (np.isfinite(want) & (want != 0)).mean() > 0.5
    n = 2 * CAP + L
    assert second_trip_blocks((n + 1) // 2) == 1954
    big_sky, big_resp = tiled(d_blk, n), tiled(d_resp, n)
    out = pj.sample_pol(em, big_sky, big_resp)
    assert_tiled(_bits(out), _bits(r_blk), "sample_pol order 1")
    del out, big_sky, big_resp


def test_sample_nearest_second_trip(pj, O, dev):
    """pj.sample_nearest, one plane -> k_sample_nearest, PXL_ZUNR = 4 points per lane: n = 2^30 + L = 1 074 741 827 points is
    2^28 + 250 001 work items, so 977 blocks take a second trip (k0 += 2^30); 17 GB of coordinates, 8.6 GB of output.  Technique
    1: the block is nearest_ref.sample's bits on a map with NaN, +-Inf, -0.0, huge and subnormal pixels (nearest_ref.points:
    ties, the seam, the pole rows, off the map, three positions not finite); the big call tiles the block."""
    shape, wcs = _fullsky(pj)
    m = N.special_map(shape, 1, 49)
    sky = N.points(O, wcs, shape, L, 50)
    em, d_blk = pj.Enmap(to_dev(m, dev), wcs), to_dev(sky, dev)
    r_blk = pj.sample_nearest(em, d_blk)
    want = N.sample(O, wcs, shape, m, sky)
    assert tuple(r_blk.shape) == (1, L) and bits_equal(r_blk.cpu().numpy(), want), "sample_nearest, the block: not the pixel's bits"
    assert np.isnan(want[0, -3:]).all() and (want[0] != 0).mean() > 0.5
    n = 4 * CAP + L
    assert second_trip_blocks((n + 3) // 4) == 977
    big = tiled(d_blk, n)
    out = pj.sample_nearest(em, big)
    assert_tiled(_bits(out[0]), _bits(r_blk[0]), "sample_nearest")
    del out, big


def test_sample_pol_nearest_second_trip(pj, O, dev):
    """pj.sample_pol_nearest -> k_sample_pol_nearest, PXL_ZUNR = 4: n = 2^30 + L points, 977 blocks take a second trip; 17 GB of
    coordinates, 17 GB of responses, 8.6 GB of output.  Technique 1: the block is nearest_ref.sample_pol's bits, NaN by position,
    on the map of special pixel values; the big call tiles the block."""
    shape, wcs = _fullsky(pj)
    m = N.special_map(shape, 3, 51)
    sky = N.points(O, wcs, shape, L, 52)
    resp = np.random.default_rng(53).normal(size=(L, 2))
    em, d_blk, d_resp = pj.Enmap(to_dev(m, dev), wcs), to_dev(sky, dev), to_dev(resp, dev)
    r_blk = pj.sample_pol_nearest(em, d_blk, d_resp)
    with np.errstate(invalid="ignore", over="ignore"):
        want = N.sample_pol(O, wcs, shape, m, sky, resp)
    same_bits(r_blk.cpu().numpy(), want, "sample_pol_nearest, the block")
    assert (np.isfinite(want) & (want != 0)).mean() > 0.5
    n = 4 * CAP + L
    assert second_trip_blocks((n + 3) // 4) == 977
    big_sky, big_resp = tiled(d_blk, n), tiled(d_resp, n)
    out = pj.sample_pol_nearest(em, big_sky, big_resp)
    assert_tiled(_bits(out), _bits(r_blk), "sample_pol_nearest")
    del out, big_sky, big_resp


# ---- the block solve and its product: per pixel -------------------------------------------------------------------------------------

def _tiled_planes(blk, npix):
    """(P, 1, npix) map whose every plane repeats the (P, L) block's plane"""
    out = torch.empty((blk.shape[0], 1, npix), dtype=blk.dtype, device=blk.device)
    for c in range(blk.shape[0]):
        out[c, 0].copy_(tiled(blk[c], npix))
    return out


def _assert_tiled_planes(out, blk, tag):
    got = out.reshape(blk.shape[0], -1)
    for c in range(blk.shape[0]):
        assert_tiled(_bits(got[c]), _bits(blk[c]), "%s, plane %d" % (tag, c))


def _solve_block(pj, dev, wcs):
    """One period of L pixels of polsolve_ref.mixed_blocks held to polsolve_ref bit for bit as tests/test_gpu_polsolve.py holds it
    (NaN by position): returns the device's (weights, rhs, solution, rcond, product) of the block, each (planes, L)."""
    from test_gpu_polsolve import _same_bits
    w6, r3 = Q.mixed_blocks(L)
    want, want_rc, info = Q.solve(w6, r3, 1e-3)
    assert info["ok"].sum() > L // 4 and (~info["ok"]).sum() > 36
    d_w, d_r = to_dev(w6, dev), to_dev(r3, dev)
    wts, rhs = pj.Enmap(d_w.view(6, 1, L), wcs), pj.Enmap(d_r.view(3, 1, L), wcs)
    x, rc = pj.pol_block_solve(rhs, wts, rcond_min=1e-3, return_rcond=True)
    y = pj.pol_block_apply(rhs, wts)
    _same_bits(x.data.cpu().numpy(), want, "solve, the block")
    _same_bits(rc.data.cpu().numpy(), want_rc, "rcond, the block")
    _same_bits(y.data.cpu().numpy(), Q.apply(w6, r3), "apply, the block")
    return d_w, d_r, x.data.view(3, L), rc.data.view(1, L), y.data.view(3, L)


def test_pol_block_odd_npix_second_trip(pj, dev):
    """k_pol_block_solve<false, true>, <false, false> and k_pol_block_apply<false>, one pixel per lane, through
    pj.pol_block_solve(return_rcond=True), pj.pol_block_solve and pj.pol_block_apply on a (1, npix) map of odd npix = 2^28 + L =
    269 435 459: 3907 blocks take a second trip (i += 2^28).  Technique 1 per pixel: the weights and right-hand sides repeat one
    block of L pixels of polsolve_ref.mixed_blocks (every special block, tie and pivot order), whose solution, rcond plane and
    product are polsolve_ref's bits; map and rcond of the big calls must tile them, as bits."""
    wcs = _fullsky(pj)[1]
    d_w, d_r, x_blk, rc_blk, y_blk = _solve_block(pj, dev, wcs)
    npix = CAP + L
    assert npix % 2 == 1 and second_trip_blocks(npix) == 3907
    wts, rhs = pj.Enmap(_tiled_planes(d_w, npix), wcs), pj.Enmap(_tiled_planes(d_r, npix), wcs)
    x, rc = pj.pol_block_solve(rhs, wts, rcond_min=1e-3, return_rcond=True)
    _assert_tiled_planes(x.data, x_blk, "solve<false, true>")
    _assert_tiled_planes(rc.data, rc_blk, "rcond<false, true>")
    del x, rc
    x = pj.pol_block_solve(rhs, wts, rcond_min=1e-3)
    _assert_tiled_planes(x.data, x_blk, "solve<false, false>")
    del x
    y = pj.pol_block_apply(rhs, wts)
    _assert_tiled_planes(y.data, y_blk, "apply<false>")
    _assert_tiled_planes(rhs.data, d_r, "the right-hand side of the out-of-place calls")
    del y, wts, rhs


def test_pol_block_even_npix_second_trip(pj, dev):
    """k_pol_block_solve<true, true>, <true, false> and k_pol_block_apply<true>, two pixels per lane, through
    pj.pol_block_solve(out=rhs, return_rcond=True), pj.pol_block_solve(out=rhs) and pj.pol_block_apply(out=x) on a (1, npix) map of
    even npix = 2^29 + L + 1 = 537 870 916 whose planes all start on 16-byte boundaries: npix / 2 = 2^28 + 500 002 work items, so
    1954 blocks take a second trip (i += 2^28 pairs).  In place, to hold memory to 26 GB of weights, 13 GB of map and the 4.3 GB
    rcond plane.  Technique 1 per pixel, as for the odd form; the in-place input is tiled afresh before each call."""
    wcs = _fullsky(pj)[1]
    d_w, d_r, x_blk, rc_blk, y_blk = _solve_block(pj, dev, wcs)
    npix = 2 * CAP + L + 1
    assert npix % 2 == 0 and second_trip_blocks(npix // 2) == 1954
    wts, rhs = pj.Enmap(_tiled_planes(d_w, npix), wcs), pj.Enmap(_tiled_planes(d_r, npix), wcs)
    assert wts.data.data_ptr() % 16 == 0 and rhs.data.data_ptr() % 16 == 0          # with even npix: every plane 16-byte aligned
    x, rc = pj.pol_block_solve(rhs, wts, rcond_min=1e-3, out=rhs, return_rcond=True)
    assert x.data.data_ptr() == rhs.data.data_ptr() and rc.data.data_ptr() % 16 == 0
    _assert_tiled_planes(x.data, x_blk, "solve<true, true> in place")
    _assert_tiled_planes(rc.data, rc_blk, "rcond<true, true>")
    del x, rc
    for c in range(3):
        rhs.data[c, 0].copy_(tiled(d_r[c], npix))
    x = pj.pol_block_solve(rhs, wts, rcond_min=1e-3, out=rhs)
    assert x.data.data_ptr() == rhs.data.data_ptr()
    _assert_tiled_planes(x.data, x_blk, "solve<true, false> in place")
    for c in range(3):
        rhs.data[c, 0].copy_(tiled(d_r[c], npix))
    y = pj.pol_block_apply(rhs, wts, out=rhs)
    assert y.data.data_ptr() == rhs.data.data_ptr()
    _assert_tiled_planes(y.data, y_blk, "apply<true> in place")
    _assert_tiled_planes(wts.data, d_w, "the weights")
    del x, y, wts, rhs


# ---- k_baseline_project<1> with baseline_len = 1: per sample in effect --------------------------------------------------------------

def _mask(rng, shape):
    """test_gpu_baseline.py's mask: a fifth of the pixels zero, a negative and a NaN pixel, the others 1 to 3"""
    nx, ny = shape
    mask = (rng.uniform(size=(ny, nx)) > 0.2).astype(float) * rng.integers(1, 4, (ny, nx))
    flat = mask.reshape(-1)
    flat[rng.integers(0, flat.size)] = -1.0
    flat[rng.integers(0, flat.size)] = np.nan
    return mask


def test_baseline_project_len_1_second_trip(pj, O, dev):
    """pj.baseline_project_pol_nearest with baseline_len = 1 -> k_baseline_project<1>, G = 1: a segment is one sample and a block
    takes 256 of them.  One detector, t0 = 0, n_chunk = n_base = 2^28 + L = 269 435 459 segments: 3907 blocks take a second trip
    (seg0 += 2^28).  Technique 1: samples, weights, amplitudes and the initial `out` repeat a block of L, with a map and a mask;
    the block's `out` is destripe_ref's bits (every baseline holds at most one term, so out[b] + w (x - s) rounds once on either
    side; destripe_ref.project itself confirms the first 5000), baselines whose sample is cut keep their bits, and the big `out`
    must tile the block's."""
    shape, wcs = _fullsky(pj)
    rng = np.random.default_rng(54)
    sky = N.points(O, wcs, shape, L, 55)
    psi = rng.uniform(0, np.pi, L)
    resp = np.stack([np.cos(2 * psi), np.sin(2 * psi)], axis=-1) * rng.uniform(0.8, 1.0, (L, 1))
    w, d, a = 10.0 ** rng.uniform(-1, 1, L), rng.normal(size=L) * 3, rng.normal(size=L) * 5
    m, mask, out0 = rng.normal(size=(3, shape[1], shape[0])), _mask(rng, shape), rng.normal(size=L)
    lay = (1, 0, 1, L)
    terms, b, size = DR.project_terms(O, wcs, shape, sky, resp, w, *lay, d=d, a=a, m=m, mask=mask)
    assert size == L and len(np.unique(b)) == len(b) and L // 2 < len(b) < L
    want = out0.copy()
    want[b] = out0[b] + terms
    head = 5000
    ref_head = DR.project(O, wcs, shape, sky[:head], resp[:head], w[:head], 1, 0, 1, head, d=d[:head], a=a[:head], m=m, mask=mask, out=out0[:head])
    assert bits_equal(ref_head[0], want[:head])
    dv = {k: to_dev(v, dev) for k, v in dict(sky=sky, resp=resp, w=w, d=d, a=a, out0=out0).items()}
    d_m, d_mask = to_dev(m, dev), to_dev(mask, dev)
    r_blk = pj.baseline_project_pol_nearest(dv["w"], dv["sky"], dv["resp"], shape, wcs, *lay, d=dv["d"], a=dv["a"], m=d_m, mask=d_mask,
                                            out=dv["out0"].clone())
    assert bits_equal(r_blk.cpu().numpy(), want), "baseline_project, the block"
    n = CAP + L
    assert second_trip_blocks(n) == 3907
    big = {k: tiled(v, n) for k, v in dv.items()}
    out = pj.baseline_project_pol_nearest(big["w"], big["sky"], big["resp"], shape, wcs, 1, 0, 1, n, d=big["d"], a=big["a"], m=d_m,
                                          mask=d_mask, out=big["out0"])
    assert_tiled(_bits(out), _bits(r_blk), "baseline_project, baseline_len 1")
    del out, big


# ================================================================================================
# 2. transposes: live points in a sea of cut points
# ================================================================================================

class Sea:
    """n = U * CAP + T points of which 3 T are live: the second trip [U CAP, n), the T points before it, and T more drawn without
    replacement from the rest of the first trip.  idx: the live indices in ascending order; second: which of them lie in the
    second trip.  sky: the live positions, uniform in pixel space (normal_ref.pixel_uniform), in index order."""

    def __init__(self, O, wcs, shape, U, seed):
        self.U, self.n = U, U * CAP + T
        self.rng = np.random.default_rng(seed)
        rest = np.sort(self.rng.choice(U * CAP - T, T, replace=False))
        self.idx = np.concatenate([rest, np.arange(U * CAP - T, self.n)])
        self.second = self.idx >= U * CAP
        assert len(np.unique(self.idx)) == 3 * T and np.all(np.diff(self.idx) > 0)
        assert self.second.sum() == T and self.n - U * CAP == T, "the second trip holds exactly T live points"
        assert self.idx[0] < (U * CAP) // 2 < self.idx[T - 1], "the drawn points spread over the first trip"
        self.sky = NR.pixel_uniform(O, wcs, shape, 3 * T, self.rng)
        self.blocks = second_trip_blocks(-(-self.n // U))

    def device(self, dev, live):
        """the (n, ...) tensor that is NaN everywhere but holds `live` at the live indices"""
        live = np.ascontiguousarray(live, dtype=np.float64)
        big = torch.full((self.n,) + live.shape[1:], NAN, dtype=torch.float64, device=dev)
        big[to_dev(self.idx, dev, np.int64)] = to_dev(live, dev)
        return big


def cpu_conditions(sea, yard, bound, what):
    """What the issue asks of the CPU before the device runs.  yard(sel) -> list of (ref, k, S) triples of the live points `sel`
    (indices into the live arrays, repeats allowed), bound(ref, k, S) the module's clause.  Returns the triples of all live points.
      * at least half of the pixels of every plane take a non-zero term from a second-trip point;
      * the yardstick without the second trip (a skipped trip), and with it counted twice (a repeated trip), each break the
        clause on at least 90 % of the pixels the second trip touches."""
    every = np.arange(3 * T)
    first, second = every[~sea.second], every[sea.second]
    full, sec, skipped = yard(every), yard(second), yard(first)
    twice = yard(np.concatenate([every, second]))
    for p, ((ref, k, S), (_r, ks, Ss), (rs, _k, _S), (rt, _k2, _S2)) in enumerate(zip(full, sec, skipped, twice)):
        planes = ref.reshape((-1,) + ref.shape[-2:])
        share = (Ss.reshape(planes.shape) > 0).reshape(len(planes), -1).mean(axis=1)
        assert share.min() >= 0.5, "%s: second-trip points reach only %.2f of the pixels with a non-zero term" % (what, share.min())
        touched = ks > 0
        b = bound(ref, k, S)
        frac = [float((np.abs(other - ref) > b)[touched].mean()) for other in (rs, rt)]
        print("%s, map %d: second trip reaches %.3f of the pixels; skipped breaks the clause on %.4f of them, repeated on %.4f" % (
            what, p, share.min(), frac[0], frac[1]))
        assert min(frac) >= 0.9, (what, frac)
        assert np.isfinite(ref).all()
    return full


def _scatter_bound(ref, k, S):
    return R.bound(k, S)


def _values(sea):
    """the module's usual random inputs of the live points: (vals, resp, w)"""
    psi = sea.rng.uniform(0, np.pi, 3 * T)
    return sea.rng.normal(size=3 * T), np.stack([np.cos(2 * psi), np.sin(2 * psi)], axis=1), 10.0 ** sea.rng.uniform(-1, 1, 3 * T)


def test_scatter_bilinear_second_trip(pj, O, dev):
    """pj.scatter_bilinear, one plane -> k_scatter_bilinear, PXL_SUNR = 4: n = 2^30 + T = 1 073 841 827 points is 2^28 + 25 001
    work items, so 98 blocks take a second trip (k0 += 2^30).  Technique 2: 300 009 live points in a sea of (NaN, NaN) positions
    with NaN values; the map against scatter_ref.scatter of the live points within k 2^-52 S."""
    shape, wcs = _fullsky(pj)
    sea = Sea(O, wcs, shape, 4, 60)
    assert sea.blocks == 98
    vals = _values(sea)[0]
    (ref, k, S), = cpu_conditions(sea, lambda s: [R.scatter(O, wcs, shape, sea.sky[s], vals[s])], _scatter_bound, "scatter_bilinear")
    d_sky, d_vals = sea.device(dev, sea.sky), sea.device(dev, vals)
    got = pj.scatter_bilinear(d_vals, d_sky, shape, wcs).data.cpu().numpy()
    R.held(got, ref[0], k[0], S[0], "scatter_bilinear, n = 2^30 + T")
    del d_sky, d_vals


def test_scatter_cubic_second_trip(pj, O, dev):
    """pj.scatter_cubic, one plane -> k_scatter_cubic, PXL_CUNR = 2: n = 2^29 + T = 536 970 915 points is 2^28 + 50 002 work items,
    so 196 blocks take a second trip (k0 += 2^29).  Technique 2; the map against scatter_cubic_ref.scatter of the live points
    within k 2^-52 S (sixteen taps per point)."""
    shape, wcs = _fullsky(pj)
    sea = Sea(O, wcs, shape, 2, 61)
    assert sea.blocks == 196
    vals = _values(sea)[0]
    (ref, k, S), = cpu_conditions(sea, lambda s: [T3.scatter(O, wcs, shape, sea.sky[s], vals[s])], _scatter_bound, "scatter_cubic")
    d_sky, d_vals = sea.device(dev, sea.sky), sea.device(dev, vals)
    got = pj.scatter_cubic(d_vals, d_sky, shape, wcs).data.cpu().numpy()
    R.held(got, ref[0], k[0], S[0], "scatter_cubic, n = 2^29 + T")
    del d_sky, d_vals


@pytest.mark.parametrize("mode", [0, 1], ids=["signal3", "weights6"])
@pytest.mark.parametrize("order", [1, 3])
def test_scatter_pol_second_trip(pj, O, dev, order, mode):
    """pj.scatter_pol (mode 0) and pj.scatter_pol_weights (mode 1), order 1 -> k_scatter_pol_bilinear<3>, <6>, PXL_SUNR = 4:
    n = 2^30 + T points, 98 blocks take a second trip; order 3 with prefiltered=True (E^T alone) -> k_scatter_pol_cubic<3>, <6>,
    PXL_CUNR = 2: n = 2^29 + T points, 196 blocks.  Technique 2, responses NaN at the cut points too; the three or six planes
    against pol_ref.scatter of the live points within k 2^-52 S."""
    shape, wcs = _fullsky(pj)
    U = 4 if order == 1 else 2
    sea = Sea(O, wcs, shape, U, 62 + 2 * order + mode)
    assert sea.blocks == (98 if order == 1 else 196)
    vals, resp, w = _values(sea)
    v = w if mode else vals
    what = "%s order %d" % ("scatter_pol_weights" if mode else "scatter_pol", order)
    (ref, k, S), = cpu_conditions(sea, lambda s: [P.scatter(O, wcs, shape, sea.sky[s], v[s], resp[s], order, mode)], _scatter_bound, what)
    d_sky, d_resp, d_v = sea.device(dev, sea.sky), sea.device(dev, resp), sea.device(dev, v)
    fn = pj.scatter_pol_weights if mode else pj.scatter_pol
    got = fn(d_v, d_sky, d_resp, shape, wcs, order=order, prefiltered=(order == 3)).data.cpu().numpy()
    assert got.shape == ref.shape == ((6 if mode else 3), shape[1], shape[0])
    R.held(got, ref, k, S, "%s, n = %d CAP + T" % (what, U))
    del d_sky, d_resp, d_v


def test_normal_pol_second_trip(pj, O, dev):
    """pj.normal_pol -> k_normal_pol_bilinear, PXL_NUNR = 1: n = 2^28 + T = 268 535 459 points, so 391 blocks take a second trip
    (k0 += 2^28).  Technique 2, weights and responses NaN at the cut points; the three planes against normal_ref.normal of the
    live points (pol_ref.scatter of w * pol_ref.sample) within k 2^-52 S."""
    shape, wcs = _fullsky(pj)
    sea = Sea(O, wcs, shape, 1, 70)
    assert sea.blocks == 391
    _vals, resp, w = _values(sea)
    x = sea.rng.normal(size=(3, shape[1], shape[0]))
    (ref, k, S), = cpu_conditions(sea, lambda s: [NR.normal(O, wcs, shape, x, sea.sky[s], resp[s], w[s])], _scatter_bound, "normal_pol")
    d_sky, d_resp, d_w = sea.device(dev, sea.sky), sea.device(dev, resp), sea.device(dev, w)
    got = pj.normal_pol(pj.Enmap(to_dev(x, dev), wcs), d_w, d_sky, d_resp).data.cpu().numpy()
    R.held(got, ref, k, S, "normal_pol, n = 2^28 + T")
    del d_sky, d_resp, d_w


def test_scatter_nearest_second_trip(pj, O, dev):
    """pj.scatter_nearest, one plane -> k_scatter_nearest, PXL_ZUNR = 4: n = 2^30 + T points, 98 blocks take a second trip.
    Technique 2; the map against nearest_ref.scatter of the live points within k 2^-52 S (one pixel per point: the second trip
    reaches 0.78 of the pixels)."""
    shape, wcs = _fullsky(pj)
    sea = Sea(O, wcs, shape, 4, 71)
    assert sea.blocks == 98
    vals = _values(sea)[0]
    (ref, k, S), = cpu_conditions(sea, lambda s: [N.scatter(O, wcs, shape, sea.sky[s], vals[s])], _scatter_bound, "scatter_nearest")
    d_sky, d_vals = sea.device(dev, sea.sky), sea.device(dev, vals)
    got = pj.scatter_nearest(d_vals, d_sky, shape, wcs).data.cpu().numpy()
    R.held(got, ref[0], k[0], S[0], "scatter_nearest, n = 2^30 + T")
    del d_sky, d_vals


@pytest.mark.parametrize("mode", [0, 1], ids=["signal3", "weights6"])
def test_scatter_pol_nearest_second_trip(pj, O, dev, mode):
    """pj.scatter_pol_nearest (mode 0) and pj.scatter_pol_weights_nearest (mode 1) -> k_scatter_pol_nearest<3>, <6>, PXL_ZUNR = 4:
    n = 2^30 + T points, 98 blocks take a second trip.  Technique 2; the planes against nearest_ref.scatter_pol of the live
    points within k 2^-52 S."""
    shape, wcs = _fullsky(pj)
    sea = Sea(O, wcs, shape, 4, 72 + mode)
    assert sea.blocks == 98
    vals, resp, w = _values(sea)
    v = w if mode else vals
    what = "scatter_pol_weights_nearest" if mode else "scatter_pol_nearest"
    (ref, k, S), = cpu_conditions(sea, lambda s: [N.scatter_pol(O, wcs, shape, sea.sky[s], v[s], resp[s], mode)], _scatter_bound, what)
    d_sky, d_resp, d_v = sea.device(dev, sea.sky), sea.device(dev, resp), sea.device(dev, v)
    fn = pj.scatter_pol_weights_nearest if mode else pj.scatter_pol_nearest
    got = fn(d_v, d_sky, d_resp, shape, wcs).data.cpu().numpy()
    R.held(got, ref, k, S, what + ", n = 2^30 + T")
    del d_sky, d_resp, d_v


def test_bin_pol_nearest_second_trip(pj, O, dev):
    """pj.bin_pol_nearest -> k_bin_pol_nearest, PXL_ZUNR = 4: n = 2^30 + T points, 98 blocks take a second trip; the largest
    allocation of the file, 17 + 17 + 8.6 + 8.6 GB of inputs.  Technique 2, d, w and the responses NaN at the cut points; rhs and
    weights against nearest_ref.bin of the live points, both within k 2^-52 S."""
    shape, wcs = _fullsky(pj)
    sea = Sea(O, wcs, shape, 4, 74)
    assert sea.blocks == 98
    d, resp, w = _values(sea)
    (r_rhs, r_w) = cpu_conditions(sea, lambda s: list(N.bin(O, wcs, shape, sea.sky[s], resp[s], d[s], w[s])), _scatter_bound, "bin_pol_nearest")
    d_sky, d_resp, d_d, d_w = sea.device(dev, sea.sky), sea.device(dev, resp), sea.device(dev, d), sea.device(dev, w)
    rhs, wts = pj.bin_pol_nearest(d_d, d_w, d_sky, d_resp, shape, wcs)
    R.held(rhs.data.cpu().numpy(), *r_rhs, "bin_pol_nearest rhs, n = 2^30 + T")
    R.held(wts.data.cpu().numpy(), *r_w, "bin_pol_nearest weights, n = 2^30 + T")
    del d_sky, d_resp, d_d, d_w


def test_baseline_bin_second_trip(pj, O, dev):
    """pj.baseline_bin_pol_nearest with d and a both and a mask -> k_baseline_bin, PXL_ZUNR = 4: one detector, t0 = 0, n_chunk = n =
    2^30 + T samples, 98 blocks take a second trip; baseline_len = 1000, so a second-trip sample's baseline index is at least
    1 073 741 > 2^20, and n_base = 1 073 842 amplitudes.  Technique 2, d and w NaN at the cut samples (a[b] is read there and
    goes nowhere).  The yardstick is destripe_ref.bin of the live samples alone, which cannot form their baselines from their
    positions in that subset, so it is given x = d - a[k // 1000] (numpy, the one rounding its Chunk makes) as its `d` and no `a`;
    rhs is held to destripe_ref.bin_bound per pixel."""
    shape, wcs = _fullsky(pj)
    sea = Sea(O, wcs, shape, 4, 75)
    assert sea.blocks == 98
    blen = 1000
    nb = DR.n_base(sea.n, blen)
    assert (4 * CAP) // blen > 1 << 20 and nb == 1_073_842
    d, resp, w = _values(sea)
    a = sea.rng.normal(size=nb) * 5
    mask = _mask(sea.rng, shape)
    x = d - a[sea.idx // blen]

    def yard(s):
        return [DR.bin(O, wcs, shape, sea.sky[s], resp[s], w[s], 1, 0, 1, len(s), d=x[s], mask=mask)]
    (ref, k, S), = cpu_conditions(sea, yard, DR.bin_bound, "baseline_bin")
    d_sky, d_resp, d_d, d_w = sea.device(dev, sea.sky), sea.device(dev, resp), sea.device(dev, d), sea.device(dev, w)
    got = pj.baseline_bin_pol_nearest(d_w, d_sky, d_resp, shape, wcs, 1, 0, blen, nb, d=d_d, a=to_dev(a, dev), mask=to_dev(mask, dev))
    got = got.data.cpu().numpy()
    err, b = np.abs(got - ref), DR.bin_bound(ref, k, S)
    assert not np.isnan(got).any(), "baseline_bin: a cut sample's NaN reached the map"
    assert np.all(err <= b), "baseline_bin: %d pixels beyond the bound, worst excess %g" % (int((err > b).sum()), float((err - b).max()))
    assert not got[k == 0].view(np.int64).any(), "baseline_bin: a pixel without an uncut sample is not +0.0"
    print("baseline_bin, n = 2^30 + T: worst error / bound = %.3g over %d pixels, max k = %d" % (float((err[b > 0] / b[b > 0]).max()), err.size, int(k.max())))
    del d_sky, d_resp, d_d, d_w


# ================================================================================================
# 3. k_baseline_project: many detectors, a chunk of a few samples
# ================================================================================================

# (baseline_len, G, the kernel's U, n_det, n_chunk, t0): t0 + n_chunk reaches 23 or 3 samples into the second baseline
PROJECT = [(1024, 256, 4, (1 << 19) + 3, 40, 1024 - 17), (65, 64, 2, (1 << 21) + 3, 10, 65 - 7), (64, 64, 1, (1 << 21) + 3, 10, 64 - 7)]


@pytest.mark.parametrize("blen,G,U,nd,nc,t0", PROJECT, ids=["len1024_G256", "len65_G64", "len64_G64"])
def test_baseline_project_many_detectors_second_trip(pj, O, dev, blen, G, U, nd, nc, t0):
    """pj.baseline_project_pol_nearest -> k_baseline_project<U>, a group of G lanes per (detector, baseline) segment, 256 / G
    segments per block.  Every detector's chunk meets two baselines (nseg = 2, n_base = 2), so there are 2 n_det segments:
      baseline_len 1024  <4>, G = 256, 1 segment per block, n_det = 2^19 + 3, n_chunk = 40, t0 = 1007: 2^20 + 6 segments = blocks,
                         6 blocks take a second trip (seg0 += 2^20) and reuse wave_sum[] / wave_hit[] behind the barrier;
      baseline_len 65    <2>, G = 64, 4 per block, n_det = 2^21 + 3, n_chunk = 10, t0 = 58: 2^22 + 6 segments, 2 blocks take a
                         second trip (seg0 += 2^22), the last with two groups past the last segment;
      baseline_len 64    <1>, G = 64, the same shape with t0 = 57.
    (With 10 samples the chunk has to start 7, not 17, before the baseline's end to meet the second baseline at all.)  Technique
    3: 2.1e7 samples, exact inputs (small integers, responses and map in quarters) as test_gpu_baseline.py's
    test_exact_inputs_give_the_yardsticks_bits, so that no sum rounds and every baseline of `out`, started from integers, must be
    the yardstick's bits: destripe_ref.project_terms' terms summed per baseline (exact in any order: asserted), which
    destripe_ref.project itself confirms on the last 40 detectors, second trip included.  About 300 detectors of the first trip
    and one of the second are cut in every sample (NaN position, d and w): their baselines keep a NaN-payload sentinel bit for
    bit.  A second call repeats the first."""
    shape, wcs = _fullsky(pj)
    nx, ny = shape
    nb, n = 2, nd * nc
    assert t0 // blen == 0 and (t0 + nc - 1) // blen == 1, "every chunk meets two baselines"
    gpb = 256 // G
    assert second_trip_blocks(2 * nd, gpb) == (6 if G == 256 else 2)
    first_second = (1 << 20) * gpb // 2                                    # the first detector whose segments wait for the second trip
    assert nd - first_second == 3
    rng = np.random.default_rng(80 + blen)
    sky = N.points(O, wcs, shape, n, 81 + blen)
    resp = rng.integers(-4, 5, (n, 2)) / 4.0
    w = rng.integers(0, 5, n).astype(float)
    d = rng.integers(-8, 9, n).astype(float)
    a = rng.integers(-8, 9, nd * nb).astype(float)
    m = rng.integers(-32, 33, (3, ny, nx)) / 4.0
    mask = _mask(rng, shape)
    out0 = rng.integers(-9, 10, nd * nb).astype(float)
    # the three detectors of the second trip sit on centres of unmasked pixels, so that the two left uncut fill all four segments
    good = rng.choice(np.flatnonzero(mask.reshape(-1) > 0), 3 * nc)
    sky[first_second * nc:] = O.pix2sky(wcs, np.stack([good % nx + 1, good // nx + 1], axis=1).astype(float), O.WRAP_NONE)
    cut = np.unique(np.concatenate([rng.choice(first_second, 300, replace=False), [first_second + 1]]))
    for arr in (sky.reshape(nd, nc, 2), w.reshape(nd, nc), d.reshape(nd, nc)):
        arr[cut] = np.nan
    out0.reshape(nd, nb)[cut] = SENTINEL
    lay = (nd, t0, blen, nb)
    terms, b, size = DR.project_terms(O, wcs, shape, sky, resp, w, *lay, d=d, a=a, m=m, mask=mask)
    # no sum rounds: every term is a multiple of 1/16 and a baseline's magnitudes add up far below 2^53 / 16
    assert size == nd * nb and np.array_equal(terms * 16, np.rint(terms * 16)) and np.abs(terms).max() * nc * 16 < 2.0 ** 52
    cnt = np.bincount(b, minlength=size)
    with np.errstate(invalid="ignore"):
        want = np.where(cnt > 0, out0 + np.bincount(b, weights=terms, minlength=size), out0)
    touched = (cnt > 0).reshape(nd, nb)
    assert not touched[cut].any() and touched[first_second:].sum() == 4 and touched.mean() > 0.9
    assert (np.abs(want[cnt > 0] - out0[cnt > 0]) > 0).mean() > 0.5
    tail = 40
    s_, b_ = slice((nd - tail) * nc, None), slice((nd - tail) * nb, None)
    ref_tail = DR.project(O, wcs, shape, sky[s_], resp[s_], w[s_], tail, t0, blen, nb, d=d[s_], a=a[b_], m=m, mask=mask, out=out0[b_])
    assert bits_equal(ref_tail[0], want[b_]), "the per-baseline sums are not destripe_ref.project's"
    args = (to_dev(w, dev), to_dev(sky, dev), to_dev(resp, dev), shape, wcs) + lay
    kw = dict(d=to_dev(d, dev), a=to_dev(a, dev), m=to_dev(m, dev), mask=to_dev(mask, dev))
    d_want = _bits(to_dev(want, dev))
    for call in ("first", "second"):
        got = pj.baseline_project_pol_nearest(*args, out=to_dev(out0, dev), **kw)
        assert torch.equal(_bits(got), d_want), "baseline_len %d, %s call: %s" % (blen, call, first_bad(_bits(got), d_want))
    got = got.cpu().numpy()
    assert np.all(got.reshape(nd, nb)[cut].view(np.uint64) == SENTINEL.view(np.uint64)), "a baseline of cut samples lost its sentinel"
