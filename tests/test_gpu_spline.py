"""Cubic B-spline path on the device (pj.spline_prefilter, pj.reproject(order=3), pj.sample(order=3) and the raw C entries)
against the numpy yardstick tests/spline_ref.py.  Every value is held to spline_ref.bound (K * eps * max|plane|, K derived
from the yardstick's own rounding error); out-of-domain values must be exactly +0.0.  Each check prints its
worst error / bound."""
import ctypes as C

import numpy as np
import pytest

import spline_ref as R
from conftest import DEG, bits_equal

torch = pytest.importorskip("torch")
from gpu_support import dev
pytestmark = pytest.mark.gpu


def _enmap(pj, dev, m, wcs):
    return pj.Enmap(torch.from_numpy(np.ascontiguousarray(m)).to(dev), wcs)


def _held(got, ref, m, what):
    r = R.worst_ratio(got, ref, m)
    print("%s: worst error / bound = %.3g" % (what, r))
    assert r <= 1.0, what
    return r


def _prefilter_check(pj, dev, m, shape, wcs, what):
    em = _enmap(pj, dev, m, wcs)
    got = pj.spline_prefilter(em).data.cpu().numpy()
    again = pj.spline_prefilter(em).data.cpu().numpy()
    assert bits_equal(got, again), what + ": two calls differ"
    _held(got, R.prefilter(m, pj.is_periodic(wcs, shape[0])), m, what)
    return got


# ---- 1. prefilter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "spikes", "constant"])
@pytest.mark.parametrize("geom", ["cc_360x181", "cc_1024x513", "fejer1_360x180", "box_80x40"])
def test_prefilter(pj, dev, geom, kind):
    shape, wcs = R.geometries(pj)[geom]
    m = R.input_map(kind, shape, seed=len(geom) * 7 + len(kind))
    got = _prefilter_check(pj, dev, m, shape, wcs, "prefilter %s %s" % (geom, kind))
    if kind == "constant":
        _held(got, m, m, "prefilter %s: coefficients of a constant are the constant" % geom)


# ---- 2. launch paths (NOTES.md lists them) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nx,ny", R.LAUNCH_SIZES)
def test_prefilter_launch_paths(pj, dev, nx, ny, periodic):
    """nx, ny at 4, round the warm-up, round one segment, round one line group, odd, narrower than one warm-up (the
    boundary rule is applied to the warm-up indices more than once)."""
    shape, wcs = R.launch_geometry(pj, nx, ny, periodic)
    assert pj.is_periodic(wcs, nx) == periodic
    m = R.launch_input(shape)
    _prefilter_check(pj, dev, m, shape, wcs, "prefilter %d x %d %s" % (nx, ny, "periodic" if periodic else "box"))


def test_prefilter_large_map(pj, dev):
    """8192 x 4097 full sky: 32 segments along RA, 17 along DEC with a partial last one, 8224 + 8704 blocks."""
    shape, wcs = pj.fullsky_geometry(2 * np.pi / 8192)
    assert shape == (8192, 4097)
    m = np.random.default_rng(8192).normal(size=(4097, 8192))
    _prefilter_check(pj, dev, m, shape, wcs, "prefilter 8192 x 4097")


# ---- 3. reprojection ---------------------------------------------------------------------------------------------------------
def _reproject_ref(O, pj, m, gin, gout):
    (si, wi), (so, wo) = gin, gout
    per = pj.is_periodic(wi, si[0])
    xs, ys = O.reproject_tables(wi, si, wo, so)
    return R.evaluate(R.prefilter(m, per), xs, ys, per), xs, ys, per


@pytest.mark.parametrize("case", ["refine_2x", "half_pixel_shift", "sub_box_onto_full_sky", "box_refined_with_margin", "cc_to_fejer1"])
def test_reproject_cubic(pj, O, dev, case):
    gin, gout = R.reproject_cases(pj)[case]
    (si, wi), (so, wo) = gin, gout
    m = R.input_map("normal", si, seed=len(case))
    ref, xs, ys, per = _reproject_ref(O, pj, m, gin, gout)
    em = _enmap(pj, dev, m, wi)
    got = pj.reproject(em, so, wo, order=3).data.cpu().numpy()
    _held(got, ref, m, "reproject order 3, %s" % case)
    outside = ~(R.in_domain(ys, si[1])[:, None] & (np.ones(len(xs), bool) if per else R.in_domain(xs, si[0]))[None, :])
    if case in ("sub_box_onto_full_sky", "box_refined_with_margin"):
        assert outside.any() and not outside.all()
    z = got[:, outside]
    assert np.array_equal(z.view(np.int64), np.zeros(z.shape, np.int64)), "out-of-domain pixels must be +0.0"
    two_step = pj.reproject(pj.spline_prefilter(em), so, wo, order=3, prefiltered=True).data.cpu().numpy()
    assert bits_equal(got, two_step)
    into = pj.Enmap(torch.full((3, so[1], so[0]), 7.0, dtype=torch.float64, device=dev), wo)
    assert pj.reproject(em, so, wo, out=into, order=3) is into and bits_equal(into.data.cpu().numpy(), got)


def test_reproject_cubic_coarsen_and_flip(pj, O, dev):
    """A 3x coarser output with DEC running downwards: the window of source rows moves by more than its height, backwards."""
    si, wi = R.geometries(pj)["cc_1024x513"]
    so = (300, 150)
    wo = pj.CarClenshawCurtis((-1.2, -1.2), (150.5, 75.5), (0.0, 0.0))
    m = R.input_map("normal", si, seed=3, nc=1)[0]
    ref, *_ = _reproject_ref(O, pj, m, (si, wi), (so, wo))
    got = pj.reproject(_enmap(pj, dev, m, wi), so, wo, order=3).data.cpu().numpy()
    assert got.shape == (150, 300)
    _held(got, ref, m, "reproject order 3, coarsen 3.4x, DEC flipped")


# ---- 4. identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["cc_360x181", "box_80x40"])
def test_identity_geometry(pj, dev, geom):
    shape, wcs = R.geometries(pj)[geom]
    m = R.input_map("normal", shape, seed=11)
    got = pj.reproject(_enmap(pj, dev, m, wcs), shape, wcs, order=3).data.cpu().numpy()
    _held(got, m, m, "identity %s" % geom)


# ---- 5. what the feature is for ---------------------------------------------------------------------------------------------
def test_band_limited_field_is_ten_times_closer_than_bilinear(pj, dev):
    shape, wcs = R.geometries(pj)["cc_360x181"]

    def field(shape, wcs):
        nx, ny = shape
        ra = (wcs.crval[0] + (np.arange(1, nx + 1) - wcs.crpix[0]) * wcs.cdelt[0]) * wcs.unit
        dec = (wcs.crval[1] + (np.arange(1, ny + 1) - wcs.crpix[1]) * wcs.cdelt[1]) * wcs.unit
        f = np.cos(3 * ra) + np.cos(10 * ra) + np.cos(20 * ra + 0.3) + np.cos(45 * ra + 1.1)
        return (np.cos(dec) ** 2)[:, None] * f[None, :]

    so, wo_aligned = pj.fullsky_geometry(0.5 * DEG)
    wo = R.shifted(wcs, 0.25, 0.0, 2)
    assert so == (720, 361)
    em = _enmap(pj, dev, field(shape, wcs), wcs)
    truth = field(so, wo)
    rms1 = float(np.sqrt(np.mean((pj.reproject(em, so, wo).data.cpu().numpy() - truth) ** 2)))
    rms3 = float(np.sqrt(np.mean((pj.reproject(em, so, wo, order=3).data.cpu().numpy() - truth) ** 2)))
    print("band-limited field: RMS error bilinear %.3g, cubic %.3g, ratio %.3g" % (rms1, rms3, rms1 / rms3))
    assert rms3 < rms1 / 10


# ---- 6. scattered sampling -----------------------------------------------------------------------------------------------------
def _sample_check(pj, O, dev, m, shape, wcs, sky, what):
    per = pj.is_periodic(wcs, shape[0])
    pix = O.sky2pix(wcs, shape, sky, safe=True)
    ref = R.evaluate_points(R.prefilter(m, per), pix[:, 0], pix[:, 1], per)
    em = _enmap(pj, dev, m, wcs)
    tsky = torch.from_numpy(np.ascontiguousarray(sky)).to(dev)
    got = pj.sample(em, tsky, order=3).cpu().numpy()
    assert got.shape == ref.shape
    _held(got, ref, m, what)
    assert bits_equal(got, pj.sample(pj.spline_prefilter(em), tsky, order=3, prefiltered=True).cpu().numpy())
    assert bits_equal(pj.sample(em, tsky).cpu().numpy(), pj.sample_bilinear(em, tsky).cpu().numpy())
    return got, pix


def test_sample_cubic_million_points(pj, O, dev):
    shape, wcs = R.geometries(pj)["cc_1024x513"]
    m = R.input_map("normal", shape, seed=5)
    sky = torch.empty((1000000, 2), dtype=torch.float64, device=dev)
    pj.fill_sphere_points_(sky, 42)
    _sample_check(pj, O, dev, m, shape, wcs, sky.cpu().numpy(), "sample order 3, 1e6 sphere points")


def test_sample_cubic_special_points(pj, O, dev):
    shape, wcs = R.geometries(pj)["cc_360x181"]
    nx, ny = shape
    m = R.input_map("normal", shape, seed=6)
    rng = np.random.default_rng(7)
    dec = rng.uniform(-1.5, 1.5, 64)
    seam = np.concatenate([np.full(16, np.pi), np.full(16, -np.pi), np.pi - rng.uniform(0, 2 * DEG, 16), -np.pi + rng.uniform(0, 2 * DEG, 16)])
    ra = rng.uniform(-np.pi, np.pi, 32)
    poles = np.concatenate([np.full(16, np.pi / 2), np.full(16, -np.pi / 2)])
    sky = np.concatenate([np.stack([seam, dec], 1), np.stack([ra, poles], 1)])
    _sample_check(pj, O, dev, m, shape, wcs, sky, "sample order 3, seam and poles")
    # pixel centres return the pixel
    ii, jj = rng.integers(1, nx + 1, 500), rng.integers(1, ny + 1, 500)
    centres = O.pix2sky(wcs, np.stack([ii, jj], 1).astype(float), O.WRAP_NONE)
    got, pix = _sample_check(pj, O, dev, m, shape, wcs, centres, "sample order 3, pixel centres")
    _held(got, m[:, jj - 1, ii - 1], m, "sample order 3 on pixel centres returns the pixel")


def test_sample_cubic_outside_a_box(pj, O, dev):
    shape, wcs = R.geometries(pj)["box_80x40"]
    m = R.input_map("normal", shape, seed=8)
    rng = np.random.default_rng(9)
    sky = np.stack([rng.uniform(-30 * DEG, 30 * DEG, 4000), rng.uniform(-15 * DEG, 15 * DEG, 4000)], 1)
    got, pix = _sample_check(pj, O, dev, m, shape, wcs, sky, "sample order 3 in and round a box")
    outside = ~(R.in_domain(pix[:, 0], shape[0]) & R.in_domain(pix[:, 1], shape[1]))
    assert 1000 < outside.sum() < 3500
    z = got[:, outside]
    assert np.array_equal(z.view(np.int64), np.zeros(z.shape, np.int64))


# ---- 7. raw ABI ------------------------------------------------------------------------------------------------------------
def test_raw_abi_rejects_before_writing(pj, dev):
    lib = pj.load_library()
    L = pj._lib
    shape, wcs = R.geometries(pj)["box_80x40"]
    nx, ny = shape
    ws = wcs.to_struct()
    bad = wcs.to_struct(); bad.cdelt[0] = 0.0
    src = torch.ones((2, ny, nx), dtype=torch.float64, device=dev)
    big = torch.full((4 * 2 * ny * nx,), -7.0, dtype=torch.float64, device=dev)
    sky = torch.zeros((10, 2), dtype=torch.float64, device=dev)
    sh = L.shape_arr((nx, ny, 2)); sho = L.shape_arr((nx, ny))
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    null = C.c_void_p(0)
    pre, rep, smp = lib.pxl_spline_prefilter_car_f64, lib.pxl_reproject_car_cubic_f64, lib.pxl_sample_car_cubic_f64
    calls = [
        pre(None, sh, p(src), p(big), st), pre(C.byref(bad), sh, p(src), p(big), st), pre(C.byref(ws), None, p(src), p(big), st),
        pre(C.byref(ws), sh, null, p(big), st), pre(C.byref(ws), sh, p(src), null, st),
        pre(C.byref(ws), L.shape_arr((3, ny, 2)), p(src), p(big), st), pre(C.byref(ws), L.shape_arr((nx, 3, 2)), p(src), p(big), st),
        pre(C.byref(ws), L.shape_arr((nx, ny, 0)), p(src), p(big), st),
        pre(C.byref(ws), sh, p(big, 0), p(big, 1), st), pre(C.byref(ws), sh, p(big, 2 * nx * ny - 1), p(big, 0), st),
        pre(C.byref(ws), sh, p(big), p(big), st),
        rep(None, sh, p(src), C.byref(ws), sho, p(big), st), rep(C.byref(ws), sh, p(src), C.byref(bad), sho, p(big), st),
        rep(C.byref(ws), None, p(src), C.byref(ws), sho, p(big), st), rep(C.byref(ws), sh, p(src), C.byref(ws), None, p(big), st),
        rep(C.byref(ws), sh, null, C.byref(ws), sho, p(big), st), rep(C.byref(ws), sh, p(src), C.byref(ws), sho, null, st),
        rep(C.byref(ws), L.shape_arr((3, ny, 2)), p(src), C.byref(ws), sho, p(big), st),
        rep(C.byref(ws), L.shape_arr((nx, 2, 2)), p(src), C.byref(ws), sho, p(big), st),
        rep(C.byref(ws), sh, p(src), C.byref(ws), L.shape_arr((0, ny)), p(big), st),
        smp(None, sh, p(src), 10, p(sky), p(big), st), smp(C.byref(bad), sh, p(src), 10, p(sky), p(big), st),
        smp(C.byref(ws), None, p(src), 10, p(sky), p(big), st), smp(C.byref(ws), sh, null, 10, p(sky), p(big), st),
        smp(C.byref(ws), sh, p(src), 10, null, p(big), st), smp(C.byref(ws), sh, p(src), 10, p(sky), null, st),
        smp(C.byref(ws), sh, p(src), -1, p(sky), p(big), st), smp(C.byref(ws), L.shape_arr((nx, 3, 2)), p(src), 10, p(sky), p(big), st),
    ]
    assert calls == [-22] * len(calls), calls
    torch.cuda.synchronize()
    assert bool((big == -7.0).all()) and bool((src == 1.0).all())
    # and the same buffers are accepted once the arguments are right
    assert pre(C.byref(ws), sh, p(src), p(big), st) == 0
    assert rep(C.byref(ws), sh, p(big), C.byref(ws), sho, p(big, 2 * nx * ny), st) == 0
    assert smp(C.byref(ws), sh, p(big), 10, p(sky), p(big, 2 * nx * ny), st) == 0
    assert smp(C.byref(ws), sh, p(big), 0, null, null, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(big).all())


def test_python_wrappers_refuse_overlap(pj, dev):
    shape, wcs = R.geometries(pj)["box_80x40"]
    buf = torch.zeros(2 * 40 * 80, dtype=torch.float64, device=dev)
    m = pj.Enmap(buf[:3200].view(40, 80), wcs)
    with pytest.raises(ValueError, match="overlaps"):
        pj.spline_prefilter(m, out=m)
    with pytest.raises(ValueError, match="overlaps"):
        pj.spline_prefilter(m, out=pj.Enmap(buf[1600:4800].view(40, 80), wcs))
    out = pj.Enmap(buf[3200:].view(40, 80), wcs)
    assert pj.spline_prefilter(m, out=out) is out
