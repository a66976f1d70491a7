"""The cubic B-spline yardstick tests/spline_ref.py against its definition and against scipy, and the host-side argument checks
of pj.reproject(order=...) / pj.sample / pj.spline_prefilter.  No device."""
import re

import numpy as np
import pytest

import spline_ref as R
from conftest import DEG, ROOT

LD = np.longdouble


def _units(a, b, m):
    pl = np.asarray(m).reshape((-1,) + np.asarray(m).shape[-2:])
    a = np.asarray(a, LD).reshape(len(pl), -1); b = np.asarray(b, LD).reshape(len(pl), -1)
    return float(max(np.abs(a[i] - b[i]).max() / (R.EPS * np.abs(pl[i]).max()) for i in range(len(pl))))


@pytest.mark.parametrize("periodic", [True, False])
def test_against_scipy(periodic):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1)
    ny, nx = 61, 96
    m = rng.normal(size=(ny, nx))
    c = R.prefilter(m, periodic)
    s = ndi.spline_filter1d(m, 3, axis=1, mode="grid-wrap" if periodic else "mirror")
    s = ndi.spline_filter1d(s, 3, axis=0, mode="mirror")
    assert np.abs(c - s).max() <= R.bound(m)[0]
    # map_coordinates without its prefilter on a hand-padded coefficient array (3 samples on every side)
    pad = 3
    cols = R.fold(np.arange(1 - pad, nx + pad + 1), nx, periodic) - 1
    rows = R.fold(np.arange(1 - pad, ny + pad + 1), ny, False) - 1
    cp = c[np.ix_(rows, cols)]
    xs = rng.uniform(0.5, nx + 0.5, 300); ys = rng.uniform(0.5, ny + 0.5, 200)
    yy, xx = np.meshgrid(ys - 1 + pad, xs - 1 + pad, indexing="ij")
    ref = ndi.map_coordinates(cp, [yy, xx], order=3, mode="constant", prefilter=False)
    got = R.evaluate(c, xs, ys, periodic)
    assert np.abs(got - ref).max() <= R.bound(m)[0]
    gp = R.evaluate_points(c, xx.ravel() + 1 - pad, yy.ravel() + 1 - pad, periodic)
    assert np.abs(gp - ref.ravel()).max() <= R.bound(m)[0]


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("shape", [(4, 4), (5, 9), (181, 360), (64, 33)])
def test_residual_of_both_systems_and_pixel_centres(shape, periodic):
    ny, nx = shape
    m = np.random.default_rng(nx).normal(size=shape)
    for dtype in (np.float64, LD):
        c = R.prefilter(m, periodic, dtype)
        assert c.dtype == dtype
        assert R.residual(c, m, periodic) <= R.bound(m)[0]
        v = R.evaluate(c, np.arange(1.0, nx + 1), np.arange(1.0, ny + 1), periodic, dtype)
        assert np.abs(v - m).max() <= R.bound(m)[0]


def test_bicubic_polynomial_is_reproduced_in_the_interior():
    ny, nx = 140, 160
    u = (np.arange(1, nx + 1) - 80.0) / 80.0; v = (np.arange(1, ny + 1) - 70.0) / 70.0
    poly = lambda a, b: (1 + a - 2 * a ** 2 + 0.5 * a ** 3) * (0.3 - b + b ** 2 + 2 * b ** 3)
    m = poly(u[None, :], v[:, None])
    rng = np.random.default_rng(2)
    xs = rng.uniform(41, nx - 40, 400); ys = rng.uniform(41, ny - 40, 300)
    got = R.evaluate(R.prefilter(m, False), xs, ys, False)
    want = poly(((xs - 80.0) / 80.0)[None, :], ((ys - 70.0) / 70.0)[:, None])
    assert np.abs(got - want).max() <= R.bound(m)[0]


def test_domain_rule_at_one_ulp():
    ny, nx = 12, 20
    m = np.random.default_rng(3).normal(size=(ny, nx)) + 3.0
    c = R.prefilter(m, False)
    for n, axis in ((nx, 0), (ny, 1)):
        lo, hi = 0.5, n + 0.5
        pts = np.array([np.nextafter(lo, -1), lo, np.nextafter(lo, 1), np.nextafter(hi, 0), hi, np.nextafter(hi, 1e9)])
        mid = np.full(6, 5.25)
        x, y = (pts, mid) if axis == 0 else (mid, pts)
        v = R.evaluate_points(c, x, y, False)
        assert v[0] == 0.0 and v[5] == 0.0 and np.all(v[1:5] != 0.0)
        sep = R.evaluate(c, x, y, False)
        assert np.array_equal(np.diag(sep), v)
    # a periodic axis has no edge in x
    cp = R.prefilter(m, True)
    assert np.all(R.evaluate_points(cp, np.array([0.2, nx + 0.9]), np.array([5.0, 5.0]), True) != 0.0)


def test_seam_roll_gives_the_same_values(pj, O):
    shape, wcs = pj.fullsky_geometry(2.0 * DEG)
    nx, ny = shape
    m = np.random.default_rng(4).normal(size=(ny, nx))
    sky = R.sphere_points(5000, 5)
    k = 37
    wr = type(wcs)(wcs.cdelt, (wcs.crpix[0] + k, wcs.crpix[1]), wcs.crval)
    mr = np.roll(m, k, axis=1)
    p0 = O.sky2pix(wcs, shape, sky, safe=True); p1 = O.sky2pix(wr, shape, sky, safe=True)
    v0 = R.evaluate_points(R.prefilter(m, True), p0[:, 0], p0[:, 1], True)
    v1 = R.evaluate_points(R.prefilter(mr, True), p1[:, 0], p1[:, 1], True)
    # the positions differ by k up to rounding (1e-13 pixel), the coefficients by the solver's rounding
    assert np.abs(v0 - v1).max() <= 1e-11 * np.abs(m).max()
    assert np.abs(np.roll(R.prefilter(m, True), k, axis=1) - R.prefilter(mr, True)).max() <= R.bound(m)[0]


def test_fold_is_applied_repeatedly():
    assert list(R.fold(np.array([-10, -1, 0, 1, 4, 5, 6, 7, 12]), 4, False)) == [2, 3, 2, 1, 4, 3, 2, 1, 2]
    assert list(R.fold(np.array([-7, 0, 5, 9]), 4, True)) == [1, 4, 1, 1]


def test_k_was_measured(pj, O):
    """K is 4 x the yardstick's own Float64 error on the GPU tests' inputs; the constants in spline_ref.py are not below it."""
    wp = we = 0.0
    G = R.geometries(pj)
    for g, (s, w) in G.items():
        per = pj.is_periodic(w, s[0])
        for kind in ("normal", "spikes", "constant"):
            m = R.input_map(kind, s, seed=len(g) * 7 + len(kind))
            wp = max(wp, _units(R.prefilter(m, per), R.prefilter(m, per, LD), m))
    for nx, ny in R.LAUNCH_SIZES:
        for per in (True, False):
            m = R.launch_input((nx, ny))
            wp = max(wp, _units(R.prefilter(m, per), R.prefilter(m, per, LD), m))
    for name, ((si, wi), (so, wo)) in R.reproject_cases(pj).items():
        per = pj.is_periodic(wi, si[0]); m = R.input_map("normal", si, seed=len(name))
        xs, ys = O.reproject_tables(wi, si, wo, so)
        we = max(we, _units(R.evaluate(R.prefilter(m, per), xs, ys, per), R.evaluate(R.prefilter(m, per, LD), xs, ys, per, LD), m))
    s, w = G["cc_1024x513"]; m = R.input_map("normal", s, seed=5)
    pix = O.sky2pix(w, s, R.sphere_points(1000000, 42), safe=True)
    we = max(we, _units(R.evaluate_points(R.prefilter(m, True), pix[:, 0], pix[:, 1], True),
                        R.evaluate_points(R.prefilter(m, True, LD), pix[:, 0], pix[:, 1], True, LD), m))
    print("yardstick Float64 against long double: prefilter %.3f, evaluation %.3f eps max|m|; K = %.1f" % (wp, we, R.K))
    assert wp <= R.MEASURED_WORST_PREFILTER and we <= R.MEASURED_WORST_EVALUATE
    assert R.K == 4.0 * max(R.MEASURED_WORST_PREFILTER, R.MEASURED_WORST_EVALUATE)
    assert wp > 0.5 * R.MEASURED_WORST_PREFILTER and we > 0.5 * R.MEASURED_WORST_EVALUATE      # and not padded either


# ---- host-side argument checks (no device) ------------------------------------------------------------------------------------
def _cpu_map(pj, dtype="float64"):
    torch = pytest.importorskip("torch")
    shape, wcs = pj.fullsky_geometry(10.0 * DEG)
    return pj.Enmap(torch.zeros((shape[1], shape[0]), dtype=getattr(torch, dtype)), wcs), shape, wcs


def test_order_must_be_1_or_3(pj):
    m, shape, wcs = _cpu_map(pj)
    for order in (0, 2, 5, "3"):
        with pytest.raises(ValueError, match="order"):
            pj.reproject(m, shape, wcs, order=order)
        with pytest.raises(ValueError, match="order"):
            pj.sample(m, None, order=order)


def test_order_3_names_its_limits(pj):
    torch = pytest.importorskip("torch")
    m, shape, wcs = _cpu_map(pj)
    tan = pj.Gnomonic(wcs.cdelt, (10.0, 10.0), (0.0, 0.0))
    with pytest.raises(ValueError, match="Gnomonic"):
        pj.reproject(m, (20, 20), tan, order=3)
    with pytest.raises(ValueError, match="Gnomonic"):
        pj.reproject(pj.Enmap(m.data, tan), shape, wcs, order=3)
    with pytest.raises(ValueError, match="Gnomonic"):
        pj.sample(pj.Enmap(m.data, tan), torch.zeros((4, 2), dtype=torch.float64), order=3)
    m32, _, _ = _cpu_map(pj, "float32")
    with pytest.raises(ValueError, match="Float32"):
        pj.reproject(m32, shape, wcs, order=3)
    with pytest.raises(ValueError, match="Float32"):
        pj.sample(m32, torch.zeros((4, 2), dtype=torch.float64), order=3)
    with pytest.raises(ValueError, match="Float32"):
        pj.spline_prefilter(m32)
    plan = object.__new__(pj.ReprojectPlan)          # a windowed plan, without the device tables its constructor makes
    plan.shape_in, plan.shape_out = (shape[0], shape[1], 1), (shape[0], shape[1])
    plan.src_rows, plan.dst_rows = (2, shape[1] - 4), (0, shape[1])
    with pytest.raises(ValueError, match="row window"):
        pj.reproject(m, shape, wcs, plan=plan, order=3)
    small = pj.Enmap(torch.zeros((3, 36), dtype=torch.float64), wcs)
    with pytest.raises(ValueError, match="4 x 4"):
        pj.spline_prefilter(small)
    with pytest.raises(ValueError, match="order=3"):
        pj.reproject(m, shape, wcs, prefiltered=True)


def test_header_and_binding_declare_the_three_entries(pj):
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pixell_hip.h").read(), flags=re.S)
    for name in ("pxl_spline_prefilter_car_f64", "pxl_reproject_car_cubic_f64", "pxl_sample_car_cubic_f64"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in pj._lib.SIGNATURES
    julia = open(ROOT + "/julia/PixellHIP.jl").read()
    for name in ("pxl_spline_prefilter_car_f64", "pxl_reproject_car_cubic_f64", "pxl_sample_car_cubic_f64"):
        assert "ccall((:%s, libpixell_hip)" % name in julia, name
    assert re.search(r"function spline_prefilter\(", julia)
    assert pj.load_library().pxl_version() == 100
