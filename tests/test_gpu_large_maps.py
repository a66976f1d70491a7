"""The pointing and map-making kernels on maps whose flat element offsets pass 2^29, 2^31 and 2^32.

Two geometries (tests/large_map_case.py), each the smallest that reaches what it is for:

  tier R  rows 1 .. 26000 of the 0.25 arcmin full sky, 86400 x 26000, periodic: jr * nx + (i - 1) alone passes 2^31 from row 24856
          on, and in a three-plane map every plane step passes 2^31 and the second passes 2^32.
  tier P  the 0.5 arcmin full sky, 43200 x 21601: in three planes 2^31 falls inside plane 2, in six planes 2^32 inside plane 4.

Nothing dense is ever built on the host.  large_map_case.Case derives bands of rows (the first 8, the last 8, 16 around every
threshold's crossing element) and a few thousand points whose taps stay in their band or off the map; the yardsticks of
tests/*_ref.py compute positions on the full geometry and index the band (row0, nrows).  tests/test_large_map_case.py shows on the
CPU that each threshold's band straddles it.

  gathers     the map is zero but for random values in the bands; the samples are held exactly as the operator's small-shape test
              holds them (bits for orders 0 and 1 and for the polarised combination, spline_ref's bound for order-3 values).
  transposes  every output plane starts from one sentinel value; inside each band scatter_ref.held applies k 2^-52 S with the
              sentinel as the initial term; outside the bands every element must still hold the sentinel's bits, counted on the
              device plane by plane.  Order-0 operators run again on small integers and dyadic responses: the yardstick's bits.
  solve       bands of polsolve_ref.mixed_blocks in zero maps: the yardstick's bits in the bands, +0.0 everywhere else.
  prefilter   spline_ref.prefilter of the band with 64 rows of zeros on each interior side (the pole is sqrt(3) - 2: 64 rows
              attenuate by 1e-36), ending at the map's own first or last row where the band does.  Further than 64 rows from a
              band every element is zero in value and, a test of its own, +0.0 in bits (the kernel stores `6 c + 0.0`: the
              recursion's negative pole made every second far zero -0.0).

Every test allocates inside try / finally, skips with both figures when the device has less free memory than it needs plus
8 GiB, and needs at most 96 GiB.  Each prints a line `large-map: ...` with the worst error over its bound, the number of elements
checked untouched, the peak device bytes and the seconds."""
import time

import numpy as np
import pytest

import destripe_ref as DR
import large_map_case as LM
import nearest_ref as N
import normal_ref as NR
import pol_ref as P
import polsolve_ref as Q
import scatter_cubic_ref as T3
import scatter_ref as R
import spline_ref as SR
from conftest import bits_equal

torch = pytest.importorskip("torch")
from gpu_support import begin_large, dev, same_bits, to_dev
pytestmark = pytest.mark.gpu

GIB = 2 ** 30
CAP_BYTES = 96 * GIB
SENT = 0.3141592653589793            # the transposes' initial value: one term of every pixel's sum
SENT_EXACT = -4097.0                 # the same for the runs on small integers, where every sum is exact
PAD = 64                             # rows of zeros around a band of the prefilter tests


_cases = {}


def _case(pj, O, tier, nc):
    """The shared, unchanged bands and points of a tier (host arrays of a few thousand points; no device memory)."""
    if (tier, nc) not in _cases:
        shape, wcs = (LM.tier_r if tier == "R" else LM.tier_p)(pj)
        _cases[tier, nc] = LM.Case(O, shape, wcs, nc, seed=nc + (10 if tier == "R" else 20))
    return _cases[tier, nc]


def _begin(dev, nbytes, what):
    """Skip unless `nbytes` plus 8 GiB are free, fail above 96 GiB; start the peak-memory and wall clocks (gpu_support.begin_large)."""
    return begin_large(dev, nbytes, what, CAP_BYTES)


def _report(what, t0, dev, ratio=None, untouched=None, extra=""):
    torch.cuda.synchronize()
    print("large-map: %s: worst error / bound %s, %s elements checked untouched, %.1f GB peak, %.1f s%s"
          % (what, "bits" if ratio is None else "%.3g" % ratio, "-" if untouched is None else "%d" % untouched,
             torch.cuda.max_memory_allocated(dev) / 1e9, time.time() - t0, extra))


def _plane_bytes(case):
    return 8 * case.shape[0] * case.shape[1]


def _fill_bands(t, case, draw):
    """Write draw(b, band) -> (planes, nrows, nx) into the band rows of the (planes, ny, nx) device tensor; returns the host arrays."""
    host = []
    for b, band in enumerate(case.bands):
        v = np.ascontiguousarray(draw(b, band), dtype=np.float64)
        t[:, band.rows] = to_dev(v, t.device).to(t.dtype)
        host.append(v)
    return host


def _normal_bands(t, case, seed):
    rng = np.random.default_rng(seed)
    return _fill_bands(t, case, lambda b, band: rng.normal(size=(t.shape[0], band.nrows, case.shape[0])))


def _bits_of(x):
    return int(np.array([x], dtype=np.float64).view(np.int64)[0])


def _count(pl, differs_from=None, rows=4096):
    """How many elements of the (ny, nx) device plane are not zero, or with differs_from (an int64 plane of bits) are not those
    bits: counted 4096 rows at a time, so that no temporary of the reduction grows with the plane."""
    n = 0
    for r in range(0, pl.shape[0], rows):
        part = pl[r:r + rows]
        n += int(torch.count_nonzero(part if differs_from is None else part != differs_from))
    return n


def _changed_outside(t, case, value, pad=0):
    """(how many elements outside the bands, widened by `pad` rows, differ from `value` in bits; how many were looked at).
    Counted on the device, plane by plane and 4096 rows at a time."""
    bits, ny = _bits_of(value), case.shape[1]
    changed = looked = 0
    for c in range(t.shape[0]):
        pl = t[c].view(torch.int64)
        n = _count(pl, bits)
        looked += pl.numel()
        for band in case.bands:
            rows = slice(max(band.row0 - pad, 0), min(band.row0 + band.nrows + pad, ny))
            n -= _count(pl[rows], bits)
            looked -= pl[rows].numel()
        changed += n
    return changed, looked


def _same_bits(got, want, what):
    """gpu_support.same_bits of the flattened values: the device's (.., ny, nx) maps against the yardstick's (.., npix)."""
    same_bits(np.reshape(got, -1), np.reshape(want, -1), what)


def _gather_check(case, got, ref_band, what):
    """got (planes, N) or (N,) for all points; ref_band(b, band) the banded yardstick of band b's points: the same bits."""
    got = np.atleast_2d(got)
    seen_zero = 0
    for b, band in enumerate(case.bands):
        want = np.atleast_2d(ref_band(b, band))
        _same_bits(got[:, case.slices[b]], want, "%s, %r" % (what, band))
        assert (want != 0).mean() > 0.5, what
        seen_zero += int((want == 0).all(axis=0).sum())
    assert seen_zero > 0, what + ": no point off the map"


def _transpose_check(O, t, case, sent, run, ref_band, exact, what):
    """Fill t with the sentinel, run(t), hold every band to ref_band(b, band, init) -> (ref, k, S) and every other element to the
    sentinel's bits.  Returns (worst error / bound, elements checked untouched)."""
    nx = case.shape[0]
    t.fill_(sent)
    run(t)
    torch.cuda.synchronize()
    worst = 0.0
    for b, band in enumerate(case.bands):
        ref, k, S = ref_band(b, band, np.full((t.shape[0], band.nrows, nx), sent))
        got = t[:, band.rows].cpu().numpy()
        assert (k > 1).any(), "%s, %r: no pixel received a term" % (what, band)
        if exact:
            assert bits_equal(got, ref), "%s, %r: exact inputs, and not the yardstick's bits" % (what, band)
        else:
            worst = max(worst, R.held(got, ref, k, S, "%s, %r" % (what, band)))
    changed, looked = _changed_outside(t, case, sent)
    assert changed == 0, "%s: %d of %d elements outside the bands lost the sentinel's bits" % (what, changed, looked)
    return worst, looked


def _point_inputs(case, seed, exact):
    """(vals (3, N), resp (N, 2), w (N,)) for all points: random, or small integers and dyadic responses (every sum exact)."""
    n = case.n_points()
    rng = np.random.default_rng(seed)
    if exact:
        return rng.integers(-8, 9, (3, n)).astype(float), rng.integers(-4, 5, (n, 2)) / 4.0, rng.integers(0, 5, n).astype(float)
    psi = rng.uniform(0, np.pi, n)
    return rng.normal(size=(3, n)), np.stack([np.cos(2 * psi), np.sin(2 * psi)], axis=1), 10.0 ** rng.uniform(-1, 1, n)


def _implied_scale(c, periodic):
    """max |plane| of the map whose spline coefficients the band c (planes, nrows, nx) would be, rows beyond the band zero: what
    spline_ref.bound takes as the size of the data.  (c[i-1] + 4 c[i] + c[i+1]) / 6 along both axes, never above max |c|."""
    z = np.zeros_like(c[:, :1])
    b = (np.concatenate([z, c[:, :-1]], axis=1) + 4 * c + np.concatenate([c[:, 1:], z], axis=1)) / 6
    lf, rt = (np.roll(b, 1, axis=2), np.roll(b, -1, axis=2)) if periodic else (b, b)
    return np.abs((lf + 4 * b + rt) / 6).reshape(c.shape[0], -1).max(axis=1)


def _cubic_held(got, want, scale, what):
    """Order-3 values against spline_ref's evaluation: K eps max|plane| per plane, as test_gpu_spline.py holds them."""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    bound = SR.K * SR.EPS * np.asarray(scale)
    ratio = float((np.abs(got - want).max(axis=1) / bound).max())
    assert ratio <= 1.0, "%s: %.3g of spline_ref's bound" % (what, ratio)
    return ratio


# ================================================================================================
# tier R: offsets inside one plane
# ================================================================================================

@pytest.mark.parametrize("nc", [1, 3])
def test_nearest_tier_r(pj, O, dev, nc):
    """sample_nearest and scatter_nearest on (nc, 26000, 86400): 18 GB (nc = 1) and 54 GB (nc = 3).  Samples: the pixel's bits,
    +0.0 off the map.  Scatter: the clause on random values, the yardstick's bits on integers, the sentinel everywhere else."""
    case = _case(pj, O, "R", nc)
    shape, wcs = case.shape, case.wcs
    t0 = _begin(dev, (nc + 0.25) * _plane_bytes(case), "nearest, nc = %d" % nc)
    t = sky = None
    try:
        t = torch.zeros((nc, shape[1], shape[0]), dtype=torch.float64, device=dev)
        sky = to_dev(case.all_sky, dev)
        m = _normal_bands(t, case, 100 + nc)
        got = pj.sample_nearest(pj.Enmap(t, wcs), sky).cpu().numpy()
        _gather_check(case, got, lambda b, band: N.sample(O, wcs, shape, m[b], case.sky[b], band.row0, band.nrows), "sample_nearest")
        for exact in (False, True):
            v = _point_inputs(case, 110 + nc, exact)[0][:nc]
            dv = to_dev(v, dev)
            worst, looked = _transpose_check(
                O, t, case, SENT_EXACT if exact else SENT, lambda out: pj.scatter_nearest(dv, sky, shape, wcs, out=out),
                lambda b, band, init: N.scatter(O, wcs, shape, case.sky[b], v[:, case.slices[b]], out=init, row0=band.row0, nrows=band.nrows),
                exact, "scatter_nearest, nc = %d" % nc)
            _report("scatter_nearest nc=%d %s" % (nc, "exact" if exact else "random"), t0, dev, None if exact else worst, looked)
    finally:
        del t, sky
        torch.cuda.empty_cache()


@pytest.mark.parametrize("nc", [1, 3])
def test_scatter_bilinear_tier_r(pj, O, dev, nc):
    """scatter_bilinear into (nc, 26000, 86400) planes of the sentinel: the clause in the bands, the sentinel's bits elsewhere."""
    case = _case(pj, O, "R", nc)
    shape, wcs = case.shape, case.wcs
    t0 = _begin(dev, (nc + 0.25) * _plane_bytes(case), "scatter_bilinear, nc = %d" % nc)
    t = sky = None
    try:
        t = torch.empty((nc, shape[1], shape[0]), dtype=torch.float64, device=dev)
        sky = to_dev(case.all_sky, dev)
        v = _point_inputs(case, 120 + nc, False)[0][:nc]
        dv = to_dev(v, dev)
        worst, looked = _transpose_check(
            O, t, case, SENT, lambda out: pj.scatter_bilinear(dv, sky, shape, wcs, out=out),
            lambda b, band, init: R.scatter(O, wcs, shape, case.sky[b], v[:, case.slices[b]], out=init, row0=band.row0, nrows=band.nrows),
            False, "scatter_bilinear, nc = %d" % nc)
        _report("scatter_bilinear nc=%d" % nc, t0, dev, worst, looked)
    finally:
        del t, sky
        torch.cuda.empty_cache()


def test_sample_bilinear_tier_r(pj, O, dev):
    """sample_bilinear on one 86400 x 26000 plane: the direct gather in Float64 and in Float32, and the row-pair copy
    (SamplePairs, 8/3 of the plane: 48 GB next to the plane's 18 GB): the oracle's bits fed the band's rows."""
    case = _case(pj, O, "R", 1)
    shape, wcs = case.shape, case.wcs
    t0 = _begin(dev, (1 + 8 / 3 + 0.1) * _plane_bytes(case), "sample_bilinear")
    t = t32 = sky = pairs = None
    try:
        t = torch.zeros((1, shape[1], shape[0]), dtype=torch.float64, device=dev)
        sky = to_dev(case.all_sky, dev)
        m = _normal_bands(t, case, 130)
        em = pj.Enmap(t, wcs)
        ref = lambda b, band: O.sample_bilinear(wcs, shape + (1,), m[b], case.sky[b], band.row0, band.nrows)
        _gather_check(case, pj.sample_bilinear(em, sky).cpu().numpy(), ref, "sample_bilinear, Float64")
        pairs = pj.SamplePairs(em)
        _gather_check(case, pj.sample_bilinear(None, sky, pairs=pairs).cpu().numpy(), ref, "sample_bilinear through SamplePairs")
        del pairs
        pairs = None
        torch.cuda.empty_cache()
        t32 = t.float()
        got = pj.sample_bilinear(pj.Enmap(t32, wcs), sky)
        assert got.dtype == torch.float32
        for b, band in enumerate(case.bands):
            want = O.sample_bilinear_f32(wcs, shape + (1,), m[b].astype(np.float32), case.sky[b], src_row0=band.row0, src_nrows=band.nrows)
            assert np.array_equal(got[:, case.slices[b]].cpu().numpy().view(np.int32), want.view(np.int32)), "sample_bilinear, Float32, %r" % band
        _report("sample_bilinear f64, pairs, f32", t0, dev)
    finally:
        del t, t32, sky, pairs
        torch.cuda.empty_cache()


def _prefilter_windows(case):
    """Per band the rows [lo, hi) of the reference map: the band and PAD rows on each side, cut at the map's own ends."""
    ny = case.shape[1]
    return [(max(b.row0 - PAD, 0), min(b.row0 + b.nrows + PAD, ny)) for b in case.bands]


_prefilter_far = {}


def _prefilter_run(pj, O, dev):
    """The device work of the two prefilter tests, done once: holds the bands to their bound and returns, per operator,
    (far elements that are not zero, far elements whose bits are not +0.0, far elements looked at) -- three integers, no tensor."""
    if _prefilter_far:
        return _prefilter_far
    case = _case(pj, O, "R", 1)
    shape, wcs = case.shape, case.wcs
    nx, ny = shape
    t0 = _begin(dev, 2.25 * _plane_bytes(case), "spline_prefilter")
    src = dst = None
    try:
        src = torch.zeros((1, ny, nx), dtype=torch.float64, device=dev)
        dst = torch.empty((1, ny, nx), dtype=torch.float64, device=dev)
        m = _normal_bands(src, case, 140)
        wins = _prefilter_windows(case)
        far = {}
        for a, b in zip(sorted(wins), sorted(wins)[1:]):
            assert a[1] <= b[0], "reference windows overlap"
        for name, op, ref_fn in (("spline_prefilter", pj.spline_prefilter, lambda g: SR.prefilter(g, True)),
                                 ("spline_prefilter_transpose", pj.spline_prefilter_transpose, lambda g: T3.prefilter_transpose(g, True))):
            dst.fill_(float("nan"))
            res = op(pj.Enmap(src, wcs), out=pj.Enmap(dst, wcs))
            assert res.data.data_ptr() == dst.data_ptr()
            worst = 0.0
            for (lo, hi), band, mb in zip(wins, case.bands, m):
                g = np.zeros((1, hi - lo, nx))
                g[:, band.row0 - lo:band.row0 - lo + band.nrows] = mb
                want = ref_fn(g)
                got = dst[:, lo:hi].cpu().numpy()
                r = SR.worst_ratio(got, want, g) if name == "spline_prefilter" else T3.worst_ratio_t(got, want, g, True)
                assert r <= 1.0, "%s, %r: %.3g of the bound" % (name, band, r)
                worst = max(worst, r)
            # beyond 64 rows from every band: zero.  A NaN left from the fill counts as not zero.
            neg = _count(dst[0].view(torch.int64))
            nz = _count(dst[0])
            looked = dst[0].numel()
            for lo, hi in wins:
                nz -= _count(dst[0, lo:hi])
                neg -= _count(dst[0, lo:hi].view(torch.int64))
                looked -= dst[0, lo:hi].numel()
            _report(name, t0, dev, worst, looked, ", %d far elements not zero, %d far elements whose bits are not +0.0" % (nz, neg))
            far[name] = (nz, neg, looked)
        _prefilter_far.update(far)
    finally:
        del src, dst
        torch.cuda.empty_cache()
    return _prefilter_far


def test_spline_prefilter_tier_r(pj, O, dev):
    """spline_prefilter and spline_prefilter_transpose of one 86400 x 26000 plane (36 GB with the output) that is zero but for
    the bands.  Each band with 64 rows either side is held to spline_ref.prefilter / scatter_cubic_ref.prefilter_transpose of
    those rows alone under test_gpu_spline.py's bound; every element further than 64 rows from a band must compare equal to zero
    (an element the kernel did not write would still hold the NaN the output was filled with)."""
    for name, (nz, _neg, looked) in _prefilter_run(pj, O, dev).items():
        assert looked > 2 ** 31
        assert nz == 0, "%s: %d of %d elements further than %d rows from every band are not zero" % (name, nz, looked, PAD)


def test_spline_prefilter_far_rows_are_plus_zero_tier_r(pj, O, dev):
    """The same run, the stricter reading: every far element is +0.0 in BITS.  Before the kernel stored `6 c + 0.0` this failed,
    and not through an offset: 1 104 537 600 of the 2 209 075 200 far elements of spline_prefilter, and as many of its
    transpose, were -0.0.  The anti-causal pass is q = z (q - p) with the pole z = sqrt(3) - 2 < 0, so over a line of +0.0
    z * (+0.0 - +0.0) = -0.0, the next step gives z * (-0.0 - +0.0) = +0.0, and the signs alternate along the line."""
    for name, (_nz, neg, looked) in _prefilter_run(pj, O, dev).items():
        assert neg == 0, "%s: %d of %d far elements are zero but not +0.0 in bits" % (name, neg, looked)


def test_cubic_tier_r(pj, O, dev):
    """sample(order=3, prefiltered=True) and scatter_cubic on one 86400 x 26000 plane.  The coefficient plane is zero but for
    random bands; the samples are held to spline_ref.evaluate_points of the band under spline_ref's bound (the data's size
    taken from the map those coefficients stand for); the scatter to the clause, the sentinel's bits elsewhere."""
    case = _case(pj, O, "R", 1)
    shape, wcs = case.shape, case.wcs
    t0 = _begin(dev, 1.25 * _plane_bytes(case), "order 3")
    t = sky = None
    try:
        t = torch.zeros((1, shape[1], shape[0]), dtype=torch.float64, device=dev)
        sky = to_dev(case.all_sky, dev)
        c = _normal_bands(t, case, 150)
        got = pj.sample(pj.Enmap(t, wcs), sky, order=3, prefiltered=True).cpu().numpy()
        worst = 0.0
        for b, band in enumerate(case.bands):
            want = P.sample_planes(O, wcs, shape, c[b], case.sky[b], 3, True, band.row0, band.nrows)
            worst = max(worst, _cubic_held(got[:, case.slices[b]], want, _implied_scale(c[b], True), "sample order 3, %r" % band))
            assert (want != 0).mean() > 0.5
            zero = (want == 0).all(axis=0)
            assert band.name != "last" or zero.any()
            assert not got[:, case.slices[b]][:, zero].view(np.int64).any(), "sample order 3, %r: off the map is not +0.0" % band
        _report("sample order 3", t0, dev, worst)
        v = _point_inputs(case, 151, False)[0][:1]
        dv = to_dev(v, dev)
        worst, looked = _transpose_check(
            O, t, case, SENT, lambda out: pj.scatter_cubic(dv, sky, shape, wcs, out=out),
            lambda b, band, init: T3.scatter(O, wcs, shape, case.sky[b], v[:, case.slices[b]], out=init, row0=band.row0, nrows=band.nrows),
            False, "scatter_cubic")
        _report("scatter_cubic", t0, dev, worst, looked)
    finally:
        del t, sky
        torch.cuda.empty_cache()


@pytest.mark.parametrize("order", [0, 1, 3])
def test_pol_tier_r(pj, O, dev, order):
    """sample_pol / scatter_pol (orders 1 and 3, prefiltered=True for 3) and sample_pol_nearest / scatter_pol_nearest (order 0) on
    the (3, 26000, 86400) IQU map, 54 GB: every plane step passes 2^31, the second 2^32.  Samples as tests/test_gpu_pol.py and
    test_gpu_nearest.py hold them: the yardstick's bits for orders 0 and 1; for order 3 the bits of pol_ref.combine of the
    device's own scalar samples, themselves under spline_ref's bound.  Transposes: the clause, the sentinel elsewhere, and for
    order 0 the yardstick's bits on exact inputs."""
    case = _case(pj, O, "R", 3)
    shape, wcs = case.shape, case.wcs
    t0 = _begin(dev, 3.25 * _plane_bytes(case), "polarised, order %d" % order)
    t = sky = None
    try:
        t = torch.zeros((3, shape[1], shape[0]), dtype=torch.float64, device=dev)
        sky = to_dev(case.all_sky, dev)
        m = _normal_bands(t, case, 160 + order)
        _vals, resp, _w = _point_inputs(case, 170 + order, False)
        dresp = to_dev(resp, dev)
        em = pj.Enmap(t, wcs)
        worst = None
        with np.errstate(invalid="ignore", over="ignore"):
            if order == 0:
                got = pj.sample_pol_nearest(em, sky, dresp).cpu().numpy()
                _gather_check(case, got, lambda b, band: N.sample_pol(O, wcs, shape, m[b], case.sky[b], resp[case.slices[b]], band.row0, band.nrows),
                              "sample_pol_nearest")
            elif order == 1:
                got = pj.sample_pol(em, sky, dresp).cpu().numpy()
                _gather_check(case, got, lambda b, band: P.sample(O, wcs, shape, m[b], case.sky[b], resp[case.slices[b]], 1, False, band.row0, band.nrows),
                              "sample_pol order 1")
            else:
                s = pj.sample(em, sky, order=3, prefiltered=True).cpu().numpy()
                worst = 0.0
                for b, band in enumerate(case.bands):
                    want = P.sample_planes(O, wcs, shape, m[b], case.sky[b], 3, True, band.row0, band.nrows)
                    worst = max(worst, _cubic_held(s[:, case.slices[b]], want, _implied_scale(m[b], True), "scalar samples of order 3, %r" % band))
                got = pj.sample_pol(em, sky, dresp, order=3, prefiltered=True).cpu().numpy()
                _same_bits(got, P.combine(s, resp), "sample_pol order 3")
                assert (got != 0).mean() > 0.5
        _report("sample_pol order %d" % order, t0, dev, worst)
        for exact in ((False, True) if order == 0 else (False,)):
            vals, resp, _w = _point_inputs(case, 180 + order, exact)
            d, dd, dresp = vals[0], to_dev(vals[0], dev), to_dev(resp, dev)
            if order == 0:
                run = lambda out: pj.scatter_pol_nearest(dd, sky, dresp, shape, wcs, out=out)
                ref = lambda b, band, init: N.scatter_pol(O, wcs, shape, case.sky[b], d[case.slices[b]], resp[case.slices[b]], 0, out=init,
                                                          row0=band.row0, nrows=band.nrows)
            else:
                run = lambda out: pj.scatter_pol(dd, sky, dresp, shape, wcs, order=order, out=out, prefiltered=order == 3)
                ref = lambda b, band, init: P.scatter(O, wcs, shape, case.sky[b], d[case.slices[b]], resp[case.slices[b]], order, 0, out=init,
                                                      row0=band.row0, nrows=band.nrows)
            worst, looked = _transpose_check(O, t, case, SENT_EXACT if exact else SENT, run, ref, exact, "scatter_pol order %d" % order)
            _report("scatter_pol order %d %s" % (order, "exact" if exact else "random"), t0, dev, None if exact else worst, looked)
    finally:
        del t, sky
        torch.cuda.empty_cache()


@pytest.mark.parametrize("blen,t_start", [(7, 3), (1024, 2 ** 31 + 1000)], ids=["b7", "b1024_t0_past_2^31"])
def test_baseline_tier_r(pj, O, dev, blen, t_start):
    """baseline_bin_pol_nearest into rhs3 and baseline_project_pol_nearest from map3, each with a mask plane, on 86400 x 26000
    (72 GB).  Four detectors; baseline_len 7 (a group of 8 lanes per segment) and 1024 (a whole block), the second in a chunk that
    starts past t0 = 2^31, where the kernels divide in 64 bits.  The mask is 1 outside the bands and, on band pixels, positive on
    four in five, 0, negative or NaN on the others.  bin: the clause from the sentinel (and the yardstick's bits on exact
    inputs), the sentinel elsewhere.  project: destripe_ref's n 2^-52 S per baseline of the exactly rounded sum, untouched
    baselines +0.0, a second call the same bits."""
    case = _case(pj, O, "R", 3)
    shape, wcs = case.shape, case.wcs
    nx, ny = shape
    nd = 4
    n = case.n_points() // nd * nd
    n_chunk = n // nd
    nb = DR.n_base(t_start + n_chunk, blen)
    lay = (nd, t_start, blen, nb)
    t0 = _begin(dev, 4.25 * _plane_bytes(case) + 16 * nd * nb, "baseline passes, baseline_len %d" % blen)
    t = mask = sky = None
    try:
        owner = np.concatenate([np.full(s.stop - s.start, b) for b, s in enumerate(case.slices)])[:n]
        all_sky = case.all_sky[:n]
        band_sky = [np.where((owner == b)[:, None], all_sky, np.nan) for b in range(len(case.bands))]      # the other bands' samples: cut
        rng = np.random.default_rng(190 + blen)
        t = torch.empty((3, ny, nx), dtype=torch.float64, device=dev)
        mask = torch.ones((1, ny, nx), dtype=torch.float64, device=dev)

        def draw_mask(b, band):
            k = (rng.uniform(size=(1, band.nrows, nx)) > 0.2) * rng.integers(1, 4, (1, band.nrows, nx)).astype(float)
            k.reshape(-1)[rng.integers(0, k.size, 200)] = np.nan
            k.reshape(-1)[rng.integers(0, k.size, 200)] = -1.0
            return k
        mk = _fill_bands(mask, case, draw_mask)
        sky = to_dev(all_sky, dev)
        for exact in (True, False):
            vals, resp, w = _point_inputs(case, 191 + blen, exact)
            d, resp, w = vals[0, :n], resp[:n], w[:n]
            a = rng.integers(-8, 9, nd * nb).astype(float) if exact else rng.normal(size=nd * nb) * 5
            dev_args = (to_dev(w, dev), sky, to_dev(resp, dev), shape, wcs) + lay
            kw = dict(d=to_dev(d, dev), a=to_dev(a, dev), mask=mask[0])
            worst, looked = _transpose_check(
                O, t, case, SENT_EXACT if exact else SENT, lambda out: pj.baseline_bin_pol_nearest(*dev_args, out=out, **kw),
                lambda b, band, init: DR.bin(O, wcs, shape, band_sky[b], resp, w, *lay, d=d, a=a, mask=mk[b][0], out=init,
                                             row0=band.row0, nrows=band.nrows),
                exact, "baseline_bin, baseline_len %d" % blen)
            _report("baseline_bin b=%d %s" % (blen, "exact" if exact else "random"), t0, dev, None if exact else worst, looked)
        # project, on the random inputs of the last round: the three planes now hold a map, zero but for the bands
        t.zero_()
        m = _normal_bands(t, case, 192 + blen)
        got = pj.baseline_project_pol_nearest(*dev_args, m=t, **kw)
        again = pj.baseline_project_pol_nearest(*dev_args, m=t, **kw)
        assert torch.equal(got.view(torch.int64), again.view(torch.int64)), "project: a second call differs in bits"
        terms, at = [], []
        for b, band in enumerate(case.bands):
            tb, bb, size = DR.project_terms(O, wcs, shape, band_sky[b], resp, w, *lay, d=d, a=a, m=m[b], mask=mk[b][0], row0=band.row0, nrows=band.nrows)
            terms.append(tb); at.append(bb)
        ref, cnt, S = DR.exact_sums(np.concatenate(at), np.concatenate(terms), size)
        got = got.cpu().numpy()
        assert got.shape == ref.shape and (cnt > 0).sum() >= nd
        err, bound = np.abs(got - ref), DR.project_bound(cnt, S)
        assert np.all(err <= bound), "project: worst excess %g" % (err - bound).max()
        assert not got[cnt == 0].view(np.int64).any(), "project: a baseline without an uncut sample is not +0.0"
        _report("baseline_project b=%d" % blen, t0, dev, float((err[bound > 0] / bound[bound > 0]).max()), int((cnt == 0).sum()))
    finally:
        del t, mask, sky
        torch.cuda.empty_cache()


# ================================================================================================
# tier P: offsets across six planes
# ================================================================================================

@pytest.mark.parametrize("order", [0, 1, 3])
def test_scatter_pol_weights_tier_p(pj, O, dev, order):
    """scatter_pol_weights (orders 1 and 3) and scatter_pol_weights_nearest into (6, 21601, 43200), 45 GB: 2^32 falls inside
    plane 4 and plane 5 lies wholly beyond it."""
    case = _case(pj, O, "P", 6)
    shape, wcs = case.shape, case.wcs
    t0 = _begin(dev, 6.25 * _plane_bytes(case), "scatter_pol_weights, order %d" % order)
    t = sky = None
    try:
        t = torch.empty((6, shape[1], shape[0]), dtype=torch.float64, device=dev)
        sky = to_dev(case.all_sky, dev)
        for exact in ((False, True) if order == 0 else (False,)):
            _vals, resp, w = _point_inputs(case, 200 + order, exact)
            dw, dresp = to_dev(w, dev), to_dev(resp, dev)
            if order == 0:
                run = lambda out: pj.scatter_pol_weights_nearest(dw, sky, dresp, shape, wcs, out=out)
                ref = lambda b, band, init: N.scatter_pol(O, wcs, shape, case.sky[b], w[case.slices[b]], resp[case.slices[b]], 1, out=init,
                                                          row0=band.row0, nrows=band.nrows)
            else:
                run = lambda out: pj.scatter_pol_weights(dw, sky, dresp, shape, wcs, order=order, out=out, prefiltered=order == 3)
                ref = lambda b, band, init: P.scatter(O, wcs, shape, case.sky[b], w[case.slices[b]], resp[case.slices[b]], order, 1, out=init,
                                                      row0=band.row0, nrows=band.nrows)
            worst, looked = _transpose_check(O, t, case, SENT_EXACT if exact else SENT, run, ref, exact, "scatter_pol_weights order %d" % order)
            _report("scatter_pol_weights order %d %s" % (order, "exact" if exact else "random"), t0, dev, None if exact else worst, looked)
    finally:
        del t, sky
        torch.cuda.empty_cache()


def test_bin_pol_nearest_tier_p(pj, O, dev):
    """bin_pol_nearest into rhs3 and weights6 of the 0.5 arcmin full sky, 67 GB: nine planes of the sentinel."""
    case = _case(pj, O, "P", 6)
    shape, wcs = case.shape, case.wcs
    nx, ny = shape
    t0 = _begin(dev, 9.25 * _plane_bytes(case), "bin_pol_nearest")
    rhs = wts = sky = None
    try:
        rhs = torch.empty((3, ny, nx), dtype=torch.float64, device=dev)
        wts = torch.empty((6, ny, nx), dtype=torch.float64, device=dev)
        sky = to_dev(case.all_sky, dev)
        for exact in (False, True):
            vals, resp, w = _point_inputs(case, 210, exact)
            d, sent = vals[0], SENT_EXACT if exact else SENT
            dd, dw, dresp = to_dev(d, dev), to_dev(w, dev), to_dev(resp, dev)
            wts.fill_(sent)
            refs = {}

            def ref(b, band, init, which):
                if b not in refs:
                    refs[b] = N.bin(O, wcs, shape, case.sky[b], resp[case.slices[b]], d[case.slices[b]], w[case.slices[b]],
                                    rhs=np.full((3, band.nrows, nx), sent), weights=np.full((6, band.nrows, nx), sent), row0=band.row0, nrows=band.nrows)
                return refs[b][which]
            worst, looked = _transpose_check(O, rhs, case, sent, lambda out: pj.bin_pol_nearest(dd, dw, sky, dresp, shape, wcs, rhs=out, weights=wts),
                                             lambda b, band, init: ref(b, band, init, 0), exact, "bin_pol_nearest, rhs")
            # the weights of the same call: held without running again
            worst6 = 0.0
            for b, band in enumerate(case.bands):
                r6, k6, S6 = ref(b, band, None, 1)
                got = wts[:, band.rows].cpu().numpy()
                if exact:
                    assert bits_equal(got, r6), "bin_pol_nearest, weights, %r: exact inputs, and not the yardstick's bits" % band
                else:
                    worst6 = max(worst6, R.held(got, r6, k6, S6, "bin_pol_nearest, weights, %r" % band))
            changed, looked6 = _changed_outside(wts, case, sent)
            assert changed == 0, "bin_pol_nearest: %d of %d weight elements outside the bands lost the sentinel's bits" % (changed, looked6)
            _report("bin_pol_nearest %s" % ("exact" if exact else "random"), t0, dev, None if exact else max(worst, worst6), looked + looked6)
    finally:
        del rhs, wts, sky
        torch.cuda.empty_cache()


def test_normal_pol_tier_p(pj, O, dev):
    """normal_pol, y += P^T W P x, with x3 (zero but for random bands) and y3 (the sentinel) on the 0.5 arcmin full sky, 45 GB."""
    case = _case(pj, O, "P", 3)
    shape, wcs = case.shape, case.wcs
    nx, ny = shape
    t0 = _begin(dev, 6.25 * _plane_bytes(case), "normal_pol")
    x = y = sky = None
    try:
        x = torch.zeros((3, ny, nx), dtype=torch.float64, device=dev)
        y = torch.empty((3, ny, nx), dtype=torch.float64, device=dev)
        sky = to_dev(case.all_sky, dev)
        m = _normal_bands(x, case, 220)
        _vals, resp, w = _point_inputs(case, 221, False)
        dw, dresp = to_dev(w, dev), to_dev(resp, dev)
        worst, looked = _transpose_check(
            O, y, case, SENT, lambda out: pj.normal_pol(pj.Enmap(x, wcs), dw, sky, dresp, out=out),
            lambda b, band, init: NR.normal(O, wcs, shape, m[b], case.sky[b], resp[case.slices[b]], w[case.slices[b]], out=init,
                                            row0=band.row0, nrows=band.nrows),
            False, "normal_pol")
        for b, band in enumerate(case.bands):
            assert bits_equal(x[:, band.rows].cpu().numpy(), m[b]), "normal_pol changed x"
        _report("normal_pol", t0, dev, worst, looked)
    finally:
        del x, y, sky
        torch.cuda.empty_cache()


def _nonzero_outside(t, case):
    return _changed_outside(t, case, 0.0)


def test_pol_block_solve_tier_p(pj, O, dev):
    """pol_block_solve and pol_block_apply on the 0.5 arcmin full sky: weights6 + rhs3 + the rcond plane, 75 GB, always in place
    (out is rhs).  npix = 933 163 200 is even and the planes are 16-byte aligned: the two-pixels-per-lane kernels, whose
    npix / 2 items pass stream_grid's 2^20 blocks of 256, so blocks take a second trip.  The scalar kernels (npix items) are
    reached with rhs viewed 8 bytes into a buffer one element longer.  The band pixels are polsolve_ref.mixed_blocks (which holds
    every special block) and everything else is the zero block: the yardstick's bits in the bands, +0.0 in every other element of
    the solution and of rcond."""
    case = _case(pj, O, "P", 6)
    shape, wcs = case.shape, case.wcs
    nx, ny = shape
    npix = nx * ny
    assert npix % 2 == 0 and npix // 2 > (1 << 20) * 256, "the vector form would not take a second grid-stride trip"
    t0 = _begin(dev, 10.25 * _plane_bytes(case), "pol_block_solve")
    wts = buf = rc = None
    try:
        wts = torch.zeros((6, ny, nx), dtype=torch.float64, device=dev)
        buf = torch.zeros((3 * npix + 1,), dtype=torch.float64, device=dev)
        assert wts.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
        blocks = [Q.mixed_blocks(band.nrows * nx, seed=b) for b, band in enumerate(case.bands)]
        _names, sw, _sr = Q.special_blocks()
        assert all(bl[0].shape[1] > sw.shape[1] + 2 for bl in blocks)
        _fill_bands(wts, case, lambda b, band: blocks[b][0].reshape(6, band.nrows, nx))
        looked = 0
        for vec in (True, False):
            rhs = (buf[:3 * npix] if vec else buf[1:]).view(3, ny, nx)
            assert (rhs.data_ptr() % 16 == 0) == vec
            erhs, ewts = pj.Enmap(rhs, wcs), pj.Enmap(wts, wcs)
            for with_rc in (True, False):
                buf.zero_()
                _fill_bands(rhs, case, lambda b, band: blocks[b][1].reshape(3, band.nrows, nx))
                if with_rc:
                    res, rcm = pj.pol_block_solve(erhs, ewts, rcond_min=1e-3, out=erhs, return_rcond=True)
                    rc = rcm.data
                    assert rc.data_ptr() % 16 == 0
                else:
                    res = pj.pol_block_solve(erhs, ewts, rcond_min=1e-3, out=erhs)
                assert res.data.data_ptr() == rhs.data_ptr()
                what = "pol_block_solve, %s form, %s rcond" % ("vector" if vec else "scalar", "with" if with_rc else "without")
                for b, band in enumerate(case.bands):
                    want, want_rc, info = Q.solve(blocks[b][0], blocks[b][1], 1e-3)
                    assert info["ok"].sum() > band.nrows * nx // 4 and (~info["ok"]).sum() > 36
                    _same_bits(rhs[:, band.rows].cpu().numpy(), want, "%s, %r" % (what, band))
                    if with_rc:
                        _same_bits(rc[band.rows].cpu().numpy(), want_rc, "%s, rcond, %r" % (what, band))
                changed, n3 = _nonzero_outside(rhs, case)
                assert changed == 0, "%s: %d of %d elements outside the bands are not +0.0" % (what, changed, n3)
                looked += n3
                if with_rc:
                    changed, n1 = _nonzero_outside(rc.view(1, ny, nx), case)
                    assert changed == 0, "%s: %d of %d rcond elements outside the bands are not +0.0" % (what, changed, n1)
                    looked += n1
                    del rcm
                    rc = None
            # the block product, in place, on the same right-hand sides
            buf.zero_()
            _fill_bands(rhs, case, lambda b, band: blocks[b][1].reshape(3, band.nrows, nx))
            res = pj.pol_block_apply(erhs, ewts, out=erhs)
            assert res.data.data_ptr() == rhs.data_ptr()
            what = "pol_block_apply, %s form" % ("vector" if vec else "scalar")
            for b, band in enumerate(case.bands):
                _same_bits(rhs[:, band.rows].cpu().numpy(), Q.apply(blocks[b][0], blocks[b][1]), "%s, %r" % (what, band))
            changed, n3 = _nonzero_outside(rhs, case)
            assert changed == 0, "%s: %d of %d elements outside the bands are not +0.0" % (what, changed, n3)
            looked += n3
            del rhs, erhs, res
        for b, band in enumerate(case.bands):
            assert bits_equal(np.nan_to_num(wts[:, band.rows].cpu().numpy()), np.nan_to_num(blocks[b][0].reshape(6, band.nrows, nx))), "the weights changed"
        _report("pol_block_solve and pol_block_apply, vector and scalar forms", t0, dev, None, looked)
    finally:
        del wts, buf, rc
        torch.cuda.empty_cache()
