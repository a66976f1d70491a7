"""pj.scatter_bilinear / pxl_scatter_car_bilinear_f64 on the device against the numpy yardstick tests/scatter_ref.py.

Every pixel of every output is compared.  Where a pixel receives at most one non-zero term the device must give the
yardstick's BITS; elsewhere the order of the atomic adds is unspecified and the pixel is held to k * 2^-52 * S (k terms,
S = sum |term|, the initial value counted as one: scatter_ref's derivation).  Two device calls are never asserted bit-equal.
Each check prints its worst error / bound."""
import ctypes as C

import numpy as np
import pytest

import scatter_ref as R
from conftest import DEG, bits_equal

torch = pytest.importorskip("torch")
import gpu_support
from gpu_support import dev, to_dev
pytestmark = pytest.mark.gpu

CHUNK = 1024          # blockDim.x * PXL_SUNR: the points one block takes per trip


def _scatter(pj, dev, shape, wcs, sky, vals, out0=None, window=None):
    """One device call; returns the resulting map as numpy (nc, nrows, nx)."""
    out = None if out0 is None else to_dev(out0, dev)
    kw = {} if window is None else {"src_rows": window, "full_shape": shape}
    res = pj.scatter_bilinear(to_dev(vals, dev), to_dev(sky, dev).reshape(-1, 2), shape, wcs, out=out, **kw)
    assert isinstance(res, pj.Enmap)
    if out is not None:
        assert res.data.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got = res.data.cpu().numpy()
    return got.reshape((-1,) + got.shape[-2:])


def _untouched_keep_their_bits(got, out0, k, what):
    idle = k == 1
    assert idle.any(), what + ": no pixel is left alone"
    assert np.array_equal(got[idle].view(np.int64), out0[idle].view(np.int64)), what + ": an untouched pixel changed"


# ---- 1. bit-exact: pixel centres of distinct pixels ---------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("geom", ["cc_360x181", "box_80x40"])
def test_pixel_centres_give_the_yardsticks_bits(pj, O, dev, geom, nc):
    shape, wcs = R.geometries(pj)[geom]
    nx, ny = shape
    rng = np.random.default_rng(nx + nc)
    pick = rng.permutation(nx * ny)[: (nx * ny * 2) // 5]             # 40 % of the pixels, each once, in random order
    pix = np.stack([pick % nx + 1.0, pick // nx + 1.0], axis=1)
    sky = O.pix2sky(wcs, pix, O.WRAP_NONE)
    idx, w = R.taps(O, wcs, shape, sky)
    assert np.array_equal(w, np.tile([1.0, 0.0, 0.0, 0.0], (len(pick), 1))), "fx = fy = 0 at every point"
    assert np.array_equal(idx[:, 0], pick)
    vals = rng.normal(size=(nc, len(pick)))
    out0 = gpu_support.out0(nc, shape[1], shape[0], 3)
    ref, k, S = R.scatter(O, wcs, shape, sky, vals, out=out0)
    assert k.max() >= 3, "pixels also take zero terms from their neighbours' cells"
    got = _scatter(pj, dev, shape, wcs, sky, vals, out0)
    assert bits_equal(got, ref), "%d pixels differ from the yardstick's bits" % int((got != ref).sum())
    _untouched_keep_their_bits(got, out0, k, geom)


# ---- 2. random points ------------------------------------------------------------------------------------------------------
_RANDOM = {}


def _random_case(pj, O, dev, geom):
    """10^6 points of fill_sphere_points_ (seed 42) with N(0, 1) values, and the yardstick of the case: computed once."""
    if geom not in _RANDOM:
        shape, wcs = R.geometries(pj)[geom]
        n = 10 ** 6
        sky = torch.empty((n, 2), dtype=torch.float64, device=dev)
        pj.fill_sphere_points_(sky, 42)
        vals = torch.empty((2, n), dtype=torch.float64, device=dev)
        pj.fill_random_(vals, 7)
        torch.cuda.synchronize()
        out0 = gpu_support.out0(2, shape[1], shape[0], 5)
        ref, k, S = R.scatter(O, wcs, shape, sky.cpu().numpy(), vals.cpu().numpy(), out=out0)
        for a in (out0, ref, k, S):
            a.setflags(write=False)
        _RANDOM[geom] = (shape, wcs, sky, vals, out0, ref, k, S)
    return _RANDOM[geom]


@pytest.mark.parametrize("geom", ["cc_360x181", "cc_1024x513"])
def test_random_points(pj, O, dev, geom):
    """977 blocks of 1024 points, the last one partial.  Measured on the CPU with numpy's uniform-on-sphere points: 98 % of
    the 65 160 pixels of the 360 x 181 map and 89 % of the 525 312 of the 1024 x 513 map have k >= 3 (medians 68 and 9)."""
    shape, wcs, sky, vals, out0, ref, k, S = _random_case(pj, O, dev, geom)
    share = float((k >= 3).mean())
    print("%s: %.1f %% of the pixels have k >= 3" % (geom, 100 * share))
    assert share >= 0.5
    runs = []
    for _ in range(2):
        out = to_dev(out0, dev)
        assert pj.scatter_bilinear(vals, sky, shape, wcs, out=out).data.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy())
        R.held(runs[-1], ref, k, S, "random points %s, call %d" % (geom, len(runs)))
    assert np.all(np.abs(runs[0] - runs[1]) <= R.bound(k, S)), "two calls differ by more than the bound"
    print("%s: %d pixels differ between two calls" % (geom, int((runs[0] != runs[1]).sum())))


# ---- 3. geometry edges -----------------------------------------------------------------------------------------------------
def _interior(O, wcs, shape, n, seed):
    rng = np.random.default_rng(seed)
    pix = np.stack([rng.uniform(2, shape[0] - 1, n), rng.uniform(2, shape[1] - 1, n)], axis=1)
    return O.pix2sky(wcs, pix, O.WRAP_NONE)


def _edge_case(pj, O, name):
    """-> (shape, wcs, sky, vals (1, n), check(idx) asserting from the yardstick that the case is what its name says)"""
    g = R.geometries(pj)
    rng = np.random.default_rng(len(name))
    if name == "seam":
        shape, wcs = g["cc_360x181"]
        nx = shape[0]
        pix = np.stack([rng.uniform(nx, nx + 1, 3000), rng.uniform(1, shape[1], 3000)], axis=1)
        sky = O.pix2sky(wcs, pix, O.WRAP_NONE)

        def check(idx):
            ok = (idx[:, 0] >= 0) & (idx[:, 1] >= 0)
            assert ok.all() and (idx[:, 0] % nx == nx - 1).all() and (idx[:, 1] % nx == 0).all(), "column 1 comes after nx"
            assert (idx[:, 1] == idx[:, 0] - (nx - 1)).all()
    elif name == "beyond_the_box_edges":
        shape, wcs = g["box_80x40"]
        nx, ny = shape
        t = rng.uniform(0, 1, 1000)
        left = np.stack([0.5 + 0.5 * t, rng.uniform(1, ny, 1000)], axis=1)
        right = np.stack([nx + 0.5 * t, rng.uniform(1, ny, 1000)], axis=1)
        below = np.stack([rng.uniform(1, nx, 1000), 0.5 + 0.5 * t], axis=1)
        above = np.stack([rng.uniform(1, nx, 1000), ny + 0.5 * t], axis=1)
        corners = np.array([[0.6, 0.7], [nx + 0.4, 0.7], [0.6, ny + 0.3], [nx + 0.4, ny + 0.3]])
        sky = O.pix2sky(wcs, np.concatenate([left, right, below, above, corners]), O.WRAP_NONE)

        def check(idx):
            drop = (idx < 0).sum(axis=1)
            assert (drop[:4000] >= 1).mean() > 0.99 and (drop[:4000] < 4).all(), "edge cells keep some taps and drop some"
            assert (drop[4000:] == 3).all(), "a corner cell keeps one tap"
            assert (idx[:1000, 0] < 0).mean() > 0.99 and (idx[1000:2000, 1] < 0).mean() > 0.99
            assert (idx[2000:3000, 0] < 0).mean() > 0.99 and (idx[3000:4000, 2] < 0).mean() > 0.99
    elif name == "pole_rows":
        shape, wcs = g["cc_360x181"]
        nx, ny = shape
        ra = rng.uniform(-np.pi, np.pi, 2000)
        sky = np.stack([ra, np.where(np.arange(2000) % 2 == 0, np.pi / 2, -np.pi / 2)], axis=1)

        def check(idx):
            rows = np.where(idx >= 0, idx // nx, -1)
            assert set(np.unique(rows[rows >= 0])) <= {0, 1, ny - 2, ny - 1} and (rows == 0).any() and (rows == ny - 1).any()
            assert (idx < 0).any(), "the row beyond a pole is not on the map"
    elif name == "outside_the_box":
        shape, wcs = g["box_80x40"]
        sky = np.stack([rng.uniform(0.5, 3.0, 2000) * np.where(np.arange(2000) % 2, 1, -1), rng.uniform(-1.5, 1.5, 2000)], axis=1)
        sky[:4] = O.pix2sky(wcs, np.array([[-0.5, 20.0], [82.5, 20.0], [40.0, -0.5], [40.0, 42.5]]), O.WRAP_NONE)

        def check(idx):
            assert (idx < 0).all()
    elif name == "non_finite_coordinates":
        shape, wcs = g["cc_360x181"]
        sky = _interior(O, wcs, shape, 1500, 1)
        sky[0::3, 0] = np.nan
        sky[1::3, 1] = np.inf
        sky[2::3] = [-np.inf, np.nan]

        def check(idx):
            assert (idx < 0).all()
    else:
        raise KeyError(name)
    return shape, wcs, sky, rng.normal(size=(1, sky.shape[0])) + 3.0, check


@pytest.mark.parametrize("name", ["seam", "beyond_the_box_edges", "pole_rows", "outside_the_box", "non_finite_coordinates"])
def test_geometry_edges(pj, O, dev, name):
    shape, wcs, sky, vals, check = _edge_case(pj, O, name)
    idx, _w = R.taps(O, wcs, shape, sky)
    check(idx)
    out0 = gpu_support.out0(1, shape[1], shape[0], 9)
    ref, k, S = R.scatter(O, wcs, shape, sky, vals, out=out0)
    got = _scatter(pj, dev, shape, wcs, sky, vals, out0)
    R.held(got, ref, k, S, name)
    _untouched_keep_their_bits(got, out0, k, name)
    if name in ("outside_the_box", "non_finite_coordinates"):
        assert k.max() == 1 and bits_equal(got, out0), "nothing may be added"


def test_nan_value_reaches_exactly_its_four_taps(pj, O, dev):
    """One NaN value at a pixel centre (weights 1, 0, 0, 0) among finite ones: all four taps of its cell become NaN, zero
    weights included, and no other pixel does."""
    shape, wcs = R.geometries(pj)["cc_360x181"]
    nx = shape[0]
    sky = _interior(O, wcs, shape, 4000, 2)
    sky[1234] = O.pix2sky(wcs, np.array([[200.0, 77.0]]), O.WRAP_NONE)[0]
    vals = np.random.default_rng(4).normal(size=(2, 4000))
    vals[1, 1234] = np.nan
    idx, w = R.taps(O, wcs, shape, sky)
    assert np.array_equal(w[1234], [1.0, 0.0, 0.0, 0.0])
    cell = sorted([76 * nx + 199, 76 * nx + 200, 77 * nx + 199, 77 * nx + 200])
    assert sorted(idx[1234]) == cell
    out0 = gpu_support.out0(2, shape[1], shape[0], 6)
    ref, k, S = R.scatter(O, wcs, shape, sky, vals, out=out0)
    got = _scatter(pj, dev, shape, wcs, sky, vals, out0)
    R.held(got, ref, k, S, "NaN value")
    assert not np.isnan(got[0]).any()
    assert sorted(np.flatnonzero(np.isnan(got[1]))) == cell


# ---- 4. row windows ----------------------------------------------------------------------------------------------------------
def test_row_windows_concatenate_to_the_whole_map(pj, O, dev):
    shape, wcs, sky, vals, out0, ref, k, S = _random_case(pj, O, dev, "cc_360x181")
    whole = to_dev(out0, dev)
    pj.scatter_bilinear(vals, sky, shape, wcs, out=whole)
    parts = []
    for row0, nrows in ((0, 60), (60, 60), (120, 61)):
        part = to_dev(out0[:, row0:row0 + nrows], dev)
        pj.scatter_bilinear(vals, sky, shape, wcs, out=part, src_rows=(row0, nrows), full_shape=shape)
        parts.append(part)
    torch.cuda.synchronize()
    strips = torch.cat(parts, dim=1).cpu().numpy()
    R.held(strips, ref, k, S, "three strips")
    assert np.all(np.abs(strips - whole.cpu().numpy()) <= R.bound(k, S))


def test_empty_window_writes_nothing(pj, dev):
    shape, wcs = R.geometries(pj)["cc_360x181"]
    lib = pj.load_library()
    sky = to_dev(R.sphere_points(5000, 1), dev)
    vals = torch.ones(5000, dtype=torch.float64, device=dev)
    guard = torch.full((4096,), 7.25, dtype=torch.float64, device=dev)
    w = wcs.to_struct()
    rc = lib.pxl_scatter_car_bilinear_f64(C.byref(w), pj._lib.shape_arr((360, 181, 1)), C.c_void_p(guard.data_ptr() + 8 * 2048), 90, 0,
                                          5000, C.c_void_p(sky.data_ptr()), C.c_void_p(vals.data_ptr()), None)
    assert rc == 0, pj._lib.last_error()
    torch.cuda.synchronize()
    assert bool((guard == 7.25).all())
    out = pj.scatter_bilinear(vals, sky, shape, wcs, src_rows=(90, 0), full_shape=shape)
    assert tuple(out.data.shape) == (0, 360)


# ---- 5. sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, CHUNK - 1, CHUNK, CHUNK + 1])
@pytest.mark.parametrize("geom", ["box_3x2", "cc_360x181"])
def test_sizes(pj, O, dev, geom, n):
    if geom == "box_3x2":
        shape, wcs = pj.geometry([[3 * DEG, -3 * DEG], [-2 * DEG, 2 * DEG]], 2.0 * DEG)
        assert shape == (3, 2)
        sky = R.box_points(O, wcs, shape, n, n + 1, margin=1.0)
    else:
        shape, wcs = R.geometries(pj)[geom]
        sky = R.sphere_points(n, n + 1)
    vals = np.random.default_rng(n).normal(size=(2, n))
    out0 = gpu_support.out0(2, shape[1], shape[0], n)
    ref, k, S = R.scatter(O, wcs, shape, sky, vals, out=out0)
    if n:
        assert k.max() > 1
    got = _scatter(pj, dev, shape, wcs, sky, vals, out0)
    R.held(got, ref, k, S, "%s n = %d" % (geom, n))
    if n == 0:
        assert bits_equal(got, out0)
    fresh = _scatter(pj, dev, shape, wcs, sky, vals[0])             # 1-D vals, out allocated: a (ny, nx) map of zeros
    ref1, k1, S1 = R.scatter(O, wcs, shape, sky, vals[0])
    R.held(fresh, ref1, k1, S1, "%s n = %d, fresh map" % (geom, n))


# ---- 6. contention ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one_cell", "scan_line"])
def test_contention(pj, O, dev, kind):
    shape, wcs = R.geometries(pj)["cc_360x181"]
    nx, ny = shape
    n = 10 ** 5
    rng = np.random.default_rng(len(kind))
    if kind == "one_cell":
        pix = np.stack([rng.uniform(100.001, 100.999, n), rng.uniform(50.001, 50.999, n)], axis=1)
    else:
        pix = np.stack([np.linspace(1.0, nx + 0.999, n), np.full(n, 90.4)], axis=1)      # scan order: neighbouring lanes, one pixel
    sky = O.pix2sky(wcs, pix, O.WRAP_NONE)
    vals = rng.normal(size=(1, n)) + 1.0
    out0 = gpu_support.out0(1, shape[1], shape[0], 8)
    ref, k, S = R.scatter(O, wcs, shape, sky, vals, out=out0)
    hit = np.flatnonzero(k.ravel() > 1)
    if kind == "one_cell":
        assert sorted(hit) == [49 * nx + 99, 49 * nx + 100, 50 * nx + 99, 50 * nx + 100] and k.max() == n + 1
    else:
        assert len(hit) == 2 * nx and k.ravel()[hit].min() > 400
    got = _scatter(pj, dev, shape, wcs, sky, vals, out0)
    R.held(got, ref, k, S, kind)
    _untouched_keep_their_bits(got, out0, k, kind)
    # the total: every term (wy * wx) * v as the device forms it, summed in longdouble, plus the initial map; each pixel's device
    # sum is within (k - 1) * 2^-53 * S of the exact sum of its terms
    idx, w = R.taps(O, wcs, shape, sky)
    assert (idx >= 0).all()
    L = np.longdouble
    want = np.sum((w * vals[0][:, None]).astype(L)) + np.sum(out0.astype(L))
    tol = float(np.sum(k.astype(L) * 2.0 ** -53 * S.astype(L)))
    gap = float(abs(np.sum(got.astype(L)) - want))
    print("%s: total off by %.3g, bound %.3g" % (kind, gap, tol))
    assert gap <= tol


# ---- 7. adjoint identity on the device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["cc_360x181", "box_80x40"])
def test_adjoint_identity(pj, O, dev, geom):
    shape, wcs = R.geometries(pj)[geom]
    rng = np.random.default_rng(len(geom))
    sky = np.concatenate([R.sphere_points(20000, 3), R.box_points(O, wcs, shape, 20000, 4)])
    m = rng.normal(size=(2, shape[1], shape[0]))
    d = rng.normal(size=(2, sky.shape[0]))
    dsky = to_dev(sky, dev)
    pm = pj.sample_bilinear(pj.Enmap(to_dev(m, dev), wcs), dsky).cpu().numpy()
    ptd = pj.scatter_bilinear(to_dev(d, dev), dsky, shape, wcs).data.cpu().numpy()
    ref, k, S = R.scatter(O, wcs, shape, sky, d)
    R.held(ptd, ref, k, S, "P^T d %s" % geom)
    gap, b = R.adjoint_gap(m, pm, d, ptd, k, S)
    print("%s: |<Pm,d> - <m,PTd>| = %.3g, bound %.3g" % (geom, gap, b))
    assert b > 0 and gap <= b


# ---- 8. raw ABI and the wrapper's refusals --------------------------------------------------------------------------------------
def test_einval_leaves_every_buffer_untouched(pj, dev):
    lib = pj.load_library()
    shape, wcs = R.geometries(pj)["cc_360x181"]
    w = wcs.to_struct()
    n = 2000
    dst = torch.full((2, 181, 360), -3.5, dtype=torch.float64, device=dev)
    sky = torch.full((n, 2), 0.25, dtype=torch.float64, device=dev)         # on the map: a call that ran would add
    vals = torch.full((2, n), 1.5, dtype=torch.float64, device=dev)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    shp = pj._lib.shape_arr((360, 181, 2))
    f = lib.pxl_scatter_car_bilinear_f64
    bad = [
        (None, shp, P(dst), 0, 181, n, P(sky), P(vals)),                                     # no WCS
        (C.byref(w), None, P(dst), 0, 181, n, P(sky), P(vals)),                              # no shape
        (C.byref(w), shp, P(dst), 0, 181, -1, P(sky), P(vals)),                              # n < 0
        (C.byref(w), pj._lib.shape_arr((360, 181, 0)), P(dst), 0, 181, n, P(sky), P(vals)),  # nc < 1
        (C.byref(w), shp, P(dst), -1, 10, n, P(sky), P(vals)),                               # window outside [0, ny]
        (C.byref(w), shp, P(dst), 0, -1, n, P(sky), P(vals)),
        (C.byref(w), shp, P(dst), 100, 82, n, P(sky), P(vals)),
        (C.byref(w), shp, None, 0, 181, n, P(sky), P(vals)),                                 # null pointers with n > 0
        (C.byref(w), shp, P(dst), 0, 181, n, None, P(vals)),
        (C.byref(w), shp, P(dst), 0, 181, n, P(sky), None),
        (C.byref(w), shp, P(dst), 0, 181, n - 1, P(sky, 8), P(vals)),                        # 2xN batch not 16-byte aligned
        (C.byref(w), shp, P(dst), 0, 181, n, P(sky), P(dst, 8 * 1000)),                      # dst overlaps vals
        (C.byref(w), shp, P(dst), 0, 181, n, P(dst, 16 * 3000), P(vals)),                    # dst overlaps the points
    ]
    for args in bad:
        assert f(*args, None) == -22, args
        assert pj._lib.last_error()
    torch.cuda.synchronize()
    assert bool((dst == -3.5).all()) and bool((sky == 0.25).all()) and bool((vals == 1.5).all())
    assert f(C.byref(w), shp, P(dst), 0, 181, 0, None, None, None) == 0                      # n = 0: nothing launched
    # and the same arguments made valid do add, on an explicit stream
    side = torch.cuda.Stream(device=dev)
    assert f(C.byref(w), shp, P(dst), 0, 181, n, P(sky), P(vals), C.c_void_p(side.cuda_stream)) == 0, pj._lib.last_error()
    side.synchronize()
    assert int((dst != -3.5).sum()) == 8


def test_wrapper_refusals(pj, dev):
    shape, wcs = R.geometries(pj)["box_80x40"]
    sky = to_dev(R.sphere_points(100, 0), dev)
    vals = torch.ones((2, 100), dtype=torch.float64, device=dev)
    out = torch.zeros((2, 40, 80), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError):
        pj.scatter_bilinear(vals.float(), sky, shape, wcs)
    with pytest.raises(ValueError):
        pj.scatter_bilinear(vals, sky, shape, wcs, out=out.float())
    with pytest.raises(ValueError):
        pj.scatter_bilinear(vals, sky, shape, pj.Gnomonic(wcs.cdelt, wcs.crpix, wcs.crval))
    with pytest.raises(ValueError):
        pj.scatter_bilinear(vals[:, :99].contiguous(), sky, shape, wcs)
    with pytest.raises(ValueError):
        pj.scatter_bilinear(vals, sky.reshape(2, 100), shape, wcs)
    with pytest.raises(ValueError):
        pj.scatter_bilinear(vals, sky, shape, wcs, out=out[:1])
    with pytest.raises(ValueError):
        pj.scatter_bilinear(vals, sky, shape, wcs, out=torch.zeros((2, 41, 80), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        pj.scatter_bilinear(vals, sky, shape, wcs, src_rows=(30, 20), full_shape=shape)
    with pytest.raises(ValueError):
        pj.scatter_bilinear(out.view(-1)[:200].view(2, 100), sky, shape, wcs, out=out)
    with pytest.raises(ValueError):
        pj.scatter_bilinear(vals, out.view(-1)[1000:1200].view(100, 2), shape, wcs, out=out)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
    assert pj.scatter_bilinear(vals, sky, shape, wcs, out=pj.Enmap(out, wcs)).data.data_ptr() == out.data_ptr()
