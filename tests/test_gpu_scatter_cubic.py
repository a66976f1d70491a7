"""The transpose of the order-3 sampler on the device against the numpy yardstick tests/scatter_cubic_ref.py:
pj.scatter_cubic / pxl_scatter_car_cubic_f64 (E^T), pj.spline_prefilter_transpose / pxl_spline_prefilter_transpose_car_f64 (F^T)
and pj.scatter(order=3) (F^T E^T).

E^T: every pixel of every output is held to k * 2^-52 * S (scatter_ref's derivation: the order of the atomic adds is
unspecified), and to the yardstick's BITS where it takes at most one non-zero term.  F^T: every value within
KT * eps * max|D^-1 g| of the direct transposed solve.  Composite and adjoint bounds: scatter_cubic_ref.composite_bound.
Each check prints its worst error / bound."""
import ctypes as C

import numpy as np
import pytest

import scatter_cubic_ref as T
import scatter_ref as R
import spline_ref as SR
from conftest import bits_equal

torch = pytest.importorskip("torch")
import gpu_support
from gpu_support import dev, to_dev
pytestmark = pytest.mark.gpu

CHUNK = 512          # blockDim.x * PXL_CUNR: the points one block takes per trip
LD = np.longdouble


def _scatter(pj, dev, shape, wcs, sky, vals, out0=None):
    """One device call of E^T; returns the resulting map as numpy (nc, ny, nx)."""
    out = None if out0 is None else to_dev(out0, dev)
    res = pj.scatter_cubic(to_dev(vals, dev), to_dev(sky, dev).reshape(-1, 2), shape, wcs, out=out)
    assert isinstance(res, pj.Enmap)
    if out is not None:
        assert res.data.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got = res.data.cpu().numpy()
    return got.reshape((-1,) + got.shape[-2:])


def _untouched_keep_their_bits(got, out0, k, what, some=True):
    idle = k == 1
    assert idle.any() or not some, what + ": no pixel is left alone"
    assert np.array_equal(got[idle].view(np.int64), out0[idle].view(np.int64)), what + ": an untouched pixel changed"


def _check(pj, O, dev, shape, wcs, sky, vals, out0, what):
    """E^T on the device against the yardstick: the bound everywhere, bits where at most one term is not zero."""
    ref, k, S = T.scatter(O, wcs, shape, sky, vals, out=out0)
    got = _scatter(pj, dev, shape, wcs, sky, vals, out0)
    R.held(got, ref, k, S, what)
    single = T.nonzero_terms(O, wcs, shape, sky, vals) <= 1
    assert np.array_equal(got[single].view(np.int64), ref[single].view(np.int64)), what + ": a pixel with one term differs in bits"
    return got, ref, k, S


def _ft(pj, dev, g, wcs):
    em = pj.Enmap(to_dev(g, dev), wcs)
    got = pj.spline_prefilter_transpose(em).data.cpu().numpy()
    assert bits_equal(got, pj.spline_prefilter_transpose(em).data.cpu().numpy()), "two calls of F^T differ"
    return got


def _ft_held(got, g, per, what):
    r = T.worst_ratio_t(got, T.prefilter_transpose(g, per), g, per)
    print("%s: worst error / bound = %.3g" % (what, r))
    assert r <= 1.0, what
    return r


# ---- 1. E^T, bit-exact cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("geom", ["cc_360x181", "box_80x40", "box_5x7"])
def test_single_point_and_sparse_centres_give_the_yardsticks_bits(pj, O, dev, geom, nc):
    shape, wcs = T.geometries(pj)[geom]
    nx, ny = shape
    rng = np.random.default_rng(nx + nc)
    # one point, anywhere on the map: sixteen pixels (fewer next to a mirrored edge), every one from one call's terms alone
    one = O.pix2sky(wcs, np.array([[rng.uniform(1, nx), rng.uniform(1, ny)]]), O.WRAP_NONE)
    v1 = rng.normal(size=(nc, 1))
    got, ref, k, S = _check(pj, O, dev, shape, wcs, one, v1, None, "%s one point" % geom)
    if geom != "box_5x7":
        assert bits_equal(got, ref) and int((got != 0).sum()) == 16 * nc
    # pixel centres five apart: the weights are (1/6, 4/6, 1/6, 0), each centre's 3 x 3 block is its own
    ii, jj = np.meshgrid(np.arange(3, nx - 1, 5), np.arange(3, ny - 1, 5))
    pick = rng.permutation(ii.size)
    sky = O.pix2sky(wcs, np.stack([ii.ravel()[pick], jj.ravel()[pick]], axis=1).astype(float), O.WRAP_NONE)
    idx, w = T.taps(O, wcs, shape, sky)
    assert np.array_equal(np.sort(w, axis=1)[:, :7], np.zeros((len(pick), 7))), "fx = fy = 0: seven taps of sixteen weigh nothing"
    vals = rng.normal(size=(nc, len(pick)))
    out0 = gpu_support.out0(nc, shape[1], shape[0], 3)
    got, ref, k, S = _check(pj, O, dev, shape, wcs, sky, vals, out0, "%s centres" % geom)
    assert bits_equal(got, ref), "%d pixels differ from the yardstick's bits" % int((got != ref).sum())
    _untouched_keep_their_bits(got, out0, k, geom, some=geom != "box_5x7")


# ---- 2. random points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["cc_360x181", "cc_1024x513"])
def test_random_points(pj, O, dev, geom):
    """10^6 sphere points: 1954 blocks of 512 points, the last one partial; tens to hundreds of adders per pixel."""
    shape, wcs = T.geometries(pj)[geom]
    n = 10 ** 6
    assert n % CHUNK != 0
    sky = torch.empty((n, 2), dtype=torch.float64, device=dev)
    pj.fill_sphere_points_(sky, 42)
    vals = torch.empty((2, n), dtype=torch.float64, device=dev)
    pj.fill_random_(vals, 7)
    torch.cuda.synchronize()
    out0 = gpu_support.out0(2, shape[1], shape[0], 5)
    ref, k, S = T.scatter(O, wcs, shape, sky.cpu().numpy(), vals.cpu().numpy(), out=out0)
    print("%s: median k = %d" % (geom, int(np.median(k))))
    assert np.median(k) >= 16
    runs = []
    for _ in range(2):
        out = to_dev(out0, dev)
        assert pj.scatter(vals, sky, shape, wcs, order=3, out=out, prefiltered=True).data.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy())
        R.held(runs[-1], ref, k, S, "random points %s, call %d" % (geom, len(runs)))
    assert np.all(np.abs(runs[0] - runs[1]) <= R.bound(k, S)), "two calls differ by more than the bound"


# ---- 3. boxes: mirrored double taps, the domain's edge exactly, points outside ------------------------------------------
def _exactly_at(O, wcs, shape, axis, target, other):
    """A sky point whose oracle sky2pix(safe=True) coordinate along `axis` is exactly `target` (the domain's edge)."""
    pix = np.array([[target, other]] if axis == 0 else [[other, target]], dtype=float)
    sky = O.pix2sky(wcs, pix, O.WRAP_NONE)
    for step in range(-200, 201):
        s = sky.copy()
        for _ in range(abs(step)):
            s[0, axis] = np.nextafter(s[0, axis], np.inf if step > 0 else -np.inf)
        if O.sky2pix(wcs, shape, s, safe=True)[0, axis] == target:
            return s[0]
    raise AssertionError("no sky coordinate lands exactly on %r" % target)


@pytest.mark.parametrize("geom", ["box_80x40", "box_4x4", "box_5x7"])
def test_box_points_with_margin(pj, O, dev, geom):
    shape, wcs = T.geometries(pj)[geom]
    nx, ny = shape
    sky = R.box_points(O, wcs, shape, 20000, nx, margin=1.5)
    edges = np.array([_exactly_at(O, wcs, shape, 0, 0.5, 2.25), _exactly_at(O, wcs, shape, 0, nx + 0.5, 2.75),
                      _exactly_at(O, wcs, shape, 1, 0.5, 1.5), _exactly_at(O, wcs, shape, 1, ny + 0.5, 3.5)])
    sky[:4] = edges
    pix = O.sky2pix(wcs, shape, sky, safe=True)
    assert pix[0, 0] == 0.5 and pix[1, 0] == nx + 0.5 and pix[2, 1] == 0.5 and pix[3, 1] == ny + 0.5
    idx, w = T.taps(O, wcs, shape, sky)
    live = idx[:, 0] >= 0
    assert live[:4].all(), "the domain is closed at both ends"
    assert 0.05 < (~live).mean() < 0.95, "the margin puts points outside"
    assert (np.array([len(set(r)) for r in idx[live]]) < 16).any(), "taps double up next to a mirrored edge"
    vals = np.random.default_rng(ny).normal(size=(3, len(sky)))
    out0 = gpu_support.out0(3, shape[1], shape[0], 9)
    _check(pj, O, dev, shape, wcs, sky, vals, out0, "%s with margin" % geom)
    # the points outside alone: nothing may be added
    got = _scatter(pj, dev, shape, wcs, sky[~live], vals[:, ~live], out0)
    assert bits_equal(got, out0), "a point outside the domain added something"


# ---- 4. seam, poles, non-finite -----------------------------------------------------------------------------------------------
def _interior(O, wcs, shape, n, seed):
    rng = np.random.default_rng(seed)
    pix = np.stack([rng.uniform(3, shape[0] - 2, n), rng.uniform(3, shape[1] - 2, n)], axis=1)
    return O.pix2sky(wcs, pix, O.WRAP_NONE)


@pytest.mark.parametrize("name", ["seam", "pole_rows", "non_finite_coordinates"])
def test_geometry_edges(pj, O, dev, name):
    shape, wcs = T.geometries(pj)["cc_360x181"]
    nx, ny = shape
    rng = np.random.default_rng(len(name))
    if name == "seam":
        x = np.concatenate([rng.uniform(nx, nx + 1, 1500), rng.uniform(0, 1, 1500)])
        sky = O.pix2sky(wcs, np.stack([x, rng.uniform(1, ny, 3000)], axis=1), O.WRAP_NONE)
    elif name == "pole_rows":
        sky = np.stack([rng.uniform(-np.pi, np.pi, 2000), np.where(np.arange(2000) % 2 == 0, np.pi / 2, -np.pi / 2)], axis=1)
    else:
        sky = _interior(O, wcs, shape, 1500, 1)
        sky[0::3, 0] = np.nan
        sky[1::3, 1] = np.inf
        sky[2::3] = [-np.inf, np.nan]
    idx, _w = T.taps(O, wcs, shape, sky)
    cols, rows = idx % nx, idx // nx
    if name == "seam":
        assert (idx >= 0).all() and ((cols == nx - 1).any(axis=1) & (cols == 0).any(axis=1)).all(), "every point's taps straddle the seam"
    elif name == "pole_rows":
        # y = 1 or ny exactly: tap rows 0 and -1 mirror to 2 and 3 (1-based), ny + 1 and ny + 2 to ny - 1 and ny - 2
        assert (idx >= 0).all() and set(np.unique(rows)) == {0, 1, 2, ny - 3, ny - 2, ny - 1}, "rows beyond a pole mirror back"
    else:
        assert (idx < 0).all()
    vals = rng.normal(size=(1, sky.shape[0])) + 3.0
    out0 = gpu_support.out0(1, shape[1], shape[0], 9)
    got, ref, k, S = _check(pj, O, dev, shape, wcs, sky, vals, out0, name)
    _untouched_keep_their_bits(got, out0, k, name)
    if name == "non_finite_coordinates":
        assert k.max() == 1 and bits_equal(got, out0), "nothing may be added"


def test_nan_value_reaches_exactly_its_sixteen_taps(pj, O, dev):
    """One NaN value at a pixel centre (seven zero weights) next to the map's lower edge, among finite ones: every folded tap
    of its 4 x 4 block becomes NaN, zero weights included, and no other pixel does."""
    shape, wcs = T.geometries(pj)["box_80x40"]
    nx = shape[0]
    sky = _interior(O, wcs, shape, 4000, 2)
    sky[1234] = O.pix2sky(wcs, np.array([[30.0, 1.0]]), O.WRAP_NONE)[0]
    vals = np.random.default_rng(4).normal(size=(2, 4000))
    vals[1, 1234] = np.nan
    idx, w = T.taps(O, wcs, shape, sky)
    assert (w[1234] == 0).sum() == 7
    cell = sorted({r * nx + c for r in (0, 1, 2) for c in (28, 29, 30, 31)})          # rows 0, 1, 2, 3 fold to 2, 1, 2, 3
    assert sorted(set(idx[1234])) == cell
    out0 = gpu_support.out0(2, shape[1], shape[0], 6)
    got, ref, k, S = _check(pj, O, dev, shape, wcs, sky, vals, out0, "NaN value")
    assert not np.isnan(got[0]).any()
    assert sorted(np.flatnonzero(np.isnan(got[1]))) == cell


# ---- 5. sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, CHUNK - 1, CHUNK, CHUNK + 1])
@pytest.mark.parametrize("geom,nc", [("box_4x4", 1), ("cc_360x181", 3)])
def test_sizes(pj, O, dev, geom, nc, n):
    shape, wcs = T.geometries(pj)[geom]
    sky = R.box_points(O, wcs, shape, n, n + 1, margin=1.0) if geom == "box_4x4" else R.sphere_points(n, n + 1)
    vals = np.random.default_rng(n).normal(size=(nc, n))
    out0 = gpu_support.out0(nc, shape[1], shape[0], n)
    got, ref, k, S = _check(pj, O, dev, shape, wcs, sky, vals, out0, "%s n = %d" % (geom, n))
    if n == 0:
        assert bits_equal(got, out0)
    else:
        assert k.max() > 1
    fresh = _scatter(pj, dev, shape, wcs, sky, vals[0])             # 1-D vals, out allocated: a (ny, nx) map of zeros
    ref1, k1, S1 = T.scatter(O, wcs, shape, sky, vals[0])
    R.held(fresh, ref1, k1, S1, "%s n = %d, fresh map" % (geom, n))


# ---- 6. contention ---------------------------------------------------------------------------------------------------------------
def test_contention_in_one_cell(pj, O, dev):
    shape, wcs = T.geometries(pj)["cc_360x181"]
    nx, ny = shape
    n = 10 ** 5
    rng = np.random.default_rng(8)
    sky = O.pix2sky(wcs, np.stack([rng.uniform(100.001, 100.999, n), rng.uniform(50.001, 50.999, n)], axis=1), O.WRAP_NONE)
    vals = rng.normal(size=(1, n)) + 1.0
    out0 = gpu_support.out0(1, shape[1], shape[0], 8)
    got, ref, k, S = _check(pj, O, dev, shape, wcs, sky, vals, out0, "one cell")
    hit = np.flatnonzero(k.ravel() > 1)
    assert sorted(hit) == sorted(r * nx + c for r in range(48, 52) for c in range(98, 102)) and k.max() == n + 1
    _untouched_keep_their_bits(got, out0, k, "one cell")
    idx, w = T.taps(O, wcs, shape, sky)
    want = np.sum((w * vals[0][:, None]).astype(LD)) + np.sum(out0.astype(LD))
    tol = float(np.sum(k.astype(LD) * 2.0 ** -53 * S.astype(LD)))
    gap = float(abs(np.sum(got.astype(LD)) - want))
    print("one cell: total off by %.3g, bound %.3g" % (gap, tol))
    assert gap <= tol


# ---- 7. F^T ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nx,ny", SR.LAUNCH_SIZES)
def test_prefilter_transpose_launch_paths(pj, dev, nx, ny, periodic):
    """The prefilter's launch-path sizes: the scaled edge n in the first tile, in a later tile whose warm-up folds back over it
    (515, 517: the third tile, a = 481), alone in a last partial tile (257), and warm-ups that mirror more than once (4 .. 10).
    Every tile that holds position 1 or n here takes the folded path.  The `interior` path (a >= 1 and a + 319 <= n) holds
    position n only for n = 544 + 256 j, as its last warm-up sample, whose weight |z|^32 = 5e-19 is below any bound: no test
    can tell a wrong doubling there, and none tries; the scaling tests the position, not the tile kind."""
    shape, wcs = SR.launch_geometry(pj, nx, ny, periodic)
    assert pj.is_periodic(wcs, nx) == periodic
    g = T.ft_launch_input(shape)
    _ft_held(_ft(pj, dev, g, wcs), g, periodic, "F^T %d x %d %s" % (nx, ny, "periodic" if periodic else "box"))


def test_prefilter_transpose_three_components(pj, dev):
    shape, wcs = T.geometries(pj)["cc_1024x513"]
    g = SR.input_map("normal", shape, seed=31, nc=3)
    got = _ft(pj, dev, g, wcs)
    _ft_held(got, g, True, "F^T 1024 x 513, three components")
    out = pj.Enmap(torch.full((3, 513, 1024), 7.0, dtype=torch.float64, device=dev), wcs)
    assert pj.spline_prefilter_transpose(pj.Enmap(to_dev(g, dev), wcs), out=out) is out and bits_equal(out.data.cpu().numpy(), got)


def test_prefilter_transpose_of_equal_rows(pj, dev):
    """A periodic map whose rows are equal: the result is the outer product of the transposed DEC solve of a constant column
    and the cyclic RA solve of one row (no D on a cyclic axis), so the RA pass is seen alone."""
    shape, wcs = T.geometries(pj)["cc_360x181"]
    g = T.equal_rows_map(shape)
    got = _ft(pj, dev, g, wcs)
    _ft_held(got, g, True, "F^T equal rows")
    ra = SR.solve_axis0(np.ascontiguousarray(g[0, :1].T), True).T          # the cyclic solve of one row
    col = T.solve_axis0_transpose(np.ones((shape[1], 1)), False)           # the transposed DEC solve of a constant
    assert np.abs(got[0] - col * ra).max() <= T.bound_t(g, True)[0]
    assert abs(col[shape[1] // 2, 0] - 1.0) < 1e-12 and abs(col[0, 0] - 1.0) > 0.1, "the transposed system is not the prefilter's at the edge rows"


def test_prefilter_transpose_nan_reach(pj, dev):
    """A NaN pixel makes outputs non-finite only within 47 lines along each axis (cyclic along RA); outside that rectangle the
    result is that of the map with the pixel replaced by 0, within the bound."""
    shape, wcs, g = T.nan_case_map(pj)
    nx, ny = shape
    c, j, i = T.NAN_CASE[1]
    clean = g.copy(); clean[c, j, i] = 0.0
    bad = g.copy(); bad[c, j, i] = np.nan
    got = _ft(pj, dev, bad, wcs)
    assert np.isfinite(got[0]).all() and not np.isfinite(got[c, j, i])
    di = np.abs(np.arange(nx) - i); di = np.minimum(di, nx - di)
    near = (np.abs(np.arange(ny) - j) <= 47)[:, None] & (di <= 47)[None, :]
    assert np.isfinite(got[c][~near]).all(), "a non-finite output more than 47 lines from the NaN pixel"
    ref = T.prefilter_transpose(clean, True)
    far = np.where(near[None], ref, got)
    far[0] = got[0]
    _ft_held(far, clean, True, "F^T outside the NaN pixel's rectangle")


# ---- 8. composite and adjoint ---------------------------------------------------------------------------------------------------
_COMPOSITE = {}


def _composite(pj, O, dev, geom):
    """The composite case of a geometry, its yardsticks and the device's P^T d: computed once."""
    if geom not in _COMPOSITE:
        shape, wcs, sky, d, m = T.composite_case(pj, O, geom)
        per = bool(O.is_periodic(wcs, shape[0]))
        g, k, S = T.scatter(O, wcs, shape, sky, d)
        ref = T.prefilter_transpose(g, per)
        cb = T.composite_bound(g, k, S, per)
        dsky, dd = to_dev(sky, dev), to_dev(d, dev)
        ptd = pj.scatter(dd, dsky, shape, wcs, order=3).data.cpu().numpy()
        for a in (g, k, S, ref, cb, ptd):
            a.setflags(write=False)
        _COMPOSITE[geom] = (shape, wcs, sky, d, m, per, g, k, S, ref, cb, dsky, dd, ptd)
    return _COMPOSITE[geom]


@pytest.mark.parametrize("geom", T.COMPOSITE)
def test_scatter_order_3(pj, O, dev, geom):
    shape, wcs, sky, d, m, per, g, k, S, ref, cb, dsky, dd, ptd = _composite(pj, O, dev, geom)
    err = np.abs(ptd - ref).reshape(2, -1).max(axis=1)
    print("scatter order 3 %s: worst error / bound = %.3g" % (geom, float((err / cb).max())))
    assert np.all(err <= cb)
    # the two steps through the public functions, and accumulation into a given map
    two = pj.spline_prefilter_transpose(pj.scatter(dd, dsky, shape, wcs, order=3, prefiltered=True)).data.cpu().numpy()
    assert np.all(np.abs(two - ref).reshape(2, -1).max(axis=1) <= cb)
    out0 = gpu_support.out0(2, shape[1], shape[0], 12)
    out = pj.Enmap(to_dev(out0, dev), wcs)
    assert pj.scatter(dd, dsky, shape, wcs, order=3, out=out) is out
    acc = out.data.cpu().numpy()
    assert np.all(np.abs(acc - (out0 + ref)).reshape(2, -1).max(axis=1) <= cb + SR.EPS * np.abs(out0 + ref).max())
    # order 1 is scatter_bilinear
    one = pj.scatter(dd, dsky, shape, wcs).data.cpu().numpy()
    r1, k1, S1 = R.scatter(O, wcs, shape, sky, d)
    R.held(one, r1, k1, S1, "scatter order 1 %s" % geom)


@pytest.mark.parametrize("geom", T.COMPOSITE)
def test_adjoint_identity(pj, O, dev, geom):
    """|<P m, d> - <m, P^T d>| <= sum_k |d_k| bound(P m) + sum_p |m_p| bound(P^T d)_p with P = pj.sample(order=3) and
    P^T = pj.scatter(order=3), dot products in long double; the pairing without D, spline_prefilter(scatter_cubic(d)), misses it."""
    shape, wcs, sky, d, m, per, g, k, S, ref, cb, dsky, dd, ptd = _composite(pj, O, dev, geom)
    pm = pj.sample(pj.Enmap(to_dev(m, dev), wcs), dsky, order=3).cpu().numpy()
    wrong = pj.spline_prefilter(pj.scatter_cubic(dd, dsky, shape, wcs)).data.cpu().numpy()
    lhs = np.sum(pm.astype(LD) * d.astype(LD))
    bound = float(np.sum(np.abs(d).sum(axis=1) * SR.bound(m)) + np.sum(np.abs(m).reshape(2, -1).sum(axis=1) * cb))
    gap = float(abs(lhs - np.sum(m.astype(LD) * ptd.astype(LD))))
    miss = float(abs(lhs - np.sum(m.astype(LD) * wrong.astype(LD))))
    scale = float(np.sum(np.abs(pm * d)))
    print("%s: |<Pm,d> - <m,PTd>| = %.3g, bound %.3g, without D %.3g (sum |Pm d| = %.3g)" % (geom, gap, bound, miss, scale))
    assert bound > 0 and gap <= bound
    assert miss > bound, "the untransposed prefilter passes the adjoint test: the test shows nothing"
    assert miss > 1e-5 * scale


# ---- 9. raw ABI and the wrappers' refusals ----------------------------------------------------------------------------------------
def test_einval_leaves_every_buffer_untouched(pj, dev):
    lib = pj.load_library()
    L = pj._lib
    shape, wcs = T.geometries(pj)["cc_360x181"]
    w = wcs.to_struct()
    bad = wcs.to_struct(); bad.cdelt[0] = 0.0
    n = 2000
    dst = torch.full((2, 181, 360), -3.5, dtype=torch.float64, device=dev)
    src = torch.full((2, 181, 360), 1.25, dtype=torch.float64, device=dev)
    sky = torch.full((n, 2), 0.25, dtype=torch.float64, device=dev)         # on the map: a call that ran would add
    vals = torch.full((2, n), 1.5, dtype=torch.float64, device=dev)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    shp = L.shape_arr((360, 181, 2))
    sc, ft = lib.pxl_scatter_car_cubic_f64, lib.pxl_spline_prefilter_transpose_car_f64
    bad_scatter = [
        (None, shp, P(dst), n, P(sky), P(vals)), (C.byref(bad), shp, P(dst), n, P(sky), P(vals)),      # WCS
        (C.byref(w), None, P(dst), n, P(sky), P(vals)),                                                 # no shape
        (C.byref(w), L.shape_arr((360, 181, 0)), P(dst), n, P(sky), P(vals)),                           # nc < 1
        (C.byref(w), L.shape_arr((3, 181, 2)), P(dst), n, P(sky), P(vals)),                             # nx < 4
        (C.byref(w), L.shape_arr((360, 3, 2)), P(dst), n, P(sky), P(vals)),                             # ny < 4
        (C.byref(w), shp, P(dst), -1, P(sky), P(vals)),                                                 # n < 0
        (C.byref(w), shp, None, n, P(sky), P(vals)), (C.byref(w), shp, P(dst), n, None, P(vals)),       # null pointers with n > 0
        (C.byref(w), shp, P(dst), n, P(sky), None),
        (C.byref(w), shp, P(dst), n - 1, P(sky, 8), P(vals)),                                           # 2xN batch not 16-byte aligned
        (C.byref(w), shp, P(dst), n, P(sky), P(dst, 8 * 1000)),                                         # dst overlaps vals
        (C.byref(w), shp, P(dst), n, P(dst, 16 * 3000), P(vals)),                                       # dst overlaps the points
    ]
    for args in bad_scatter:
        assert sc(*args, None) == -22, args
        assert L.last_error()
    bad_ft = [
        (None, shp, P(src), P(dst)), (C.byref(bad), shp, P(src), P(dst)), (C.byref(w), None, P(src), P(dst)),
        (C.byref(w), shp, None, P(dst)), (C.byref(w), shp, P(src), None),
        (C.byref(w), L.shape_arr((3, 181, 2)), P(src), P(dst)), (C.byref(w), L.shape_arr((360, 3, 2)), P(src), P(dst)),
        (C.byref(w), L.shape_arr((360, 181, 0)), P(src), P(dst)),
        (C.byref(w), shp, P(dst), P(dst)),                                                              # dst is src
        (C.byref(w), L.shape_arr((360, 181, 1)), P(dst), P(dst, 8 * (360 * 181 - 1))),                  # one element shared
        (C.byref(w), L.shape_arr((360, 181, 1)), P(dst, 8 * 360), P(dst)),
    ]
    for args in bad_ft:
        assert ft(*args, None) == -22, args
        assert L.last_error()
    torch.cuda.synchronize()
    assert bool((dst == -3.5).all()) and bool((sky == 0.25).all()) and bool((vals == 1.5).all()) and bool((src == 1.25).all())
    assert sc(C.byref(w), shp, P(dst), 0, None, None, None) == 0                                        # n = 0: nothing launched
    assert sc(C.byref(w), shp, None, 0, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((dst == -3.5).all())
    # and the same arguments made valid do their work, on an explicit stream
    side = torch.cuda.Stream(device=dev)
    st = C.c_void_p(side.cuda_stream)
    assert sc(C.byref(w), shp, P(dst), n, P(sky), P(vals), st) == 0, L.last_error()
    side.synchronize()
    assert int((dst != -3.5).sum()) == 2 * 16
    assert ft(C.byref(w), shp, P(src), P(dst), st) == 0, L.last_error()
    side.synchronize()
    assert bool(torch.isfinite(dst).all()) and not bool((dst == -3.5).any()) and bool((src == 1.25).all())


def test_wrapper_refusals(pj, dev):
    shape, wcs = T.geometries(pj)["box_80x40"]
    sky = to_dev(R.sphere_points(100, 0), dev)
    vals = torch.ones((2, 100), dtype=torch.float64, device=dev)
    out = torch.zeros((2, 40, 80), dtype=torch.float64, device=dev)
    tan = pj.Gnomonic(wcs.cdelt, wcs.crpix, wcs.crval)
    for kw in ({"order": 3}, {"order": 3, "prefiltered": True}):
        with pytest.raises(ValueError, match="Float64"):
            pj.scatter(vals.float(), sky, shape, wcs, **kw)
        with pytest.raises(ValueError, match="Float64"):
            pj.scatter(vals, sky, shape, wcs, out=out.float(), **kw)
        with pytest.raises(ValueError, match="CAR only"):
            pj.scatter(vals, sky, shape, tan, **kw)
        with pytest.raises(ValueError, match="4 x 4"):
            pj.scatter(vals, sky, (80, 3), wcs, **kw)
        with pytest.raises(ValueError):
            pj.scatter(vals[:, :99].contiguous(), sky, shape, wcs, **kw)
        with pytest.raises(ValueError):
            pj.scatter(vals, sky.reshape(2, 100), shape, wcs, **kw)
        with pytest.raises(ValueError):
            pj.scatter(vals, sky, shape, wcs, out=out[:1], **kw)
    with pytest.raises(ValueError, match="order must be 1"):
        pj.scatter(vals, sky, shape, wcs, order=2)
    with pytest.raises(ValueError, match="overlaps"):
        pj.scatter_cubic(out.view(-1)[:200].view(2, 100), sky, shape, wcs, out=out)
    with pytest.raises(ValueError, match="overlaps"):
        pj.scatter_cubic(vals, out.view(-1)[1000:1200].view(100, 2), shape, wcs, out=out)
    m = pj.Enmap(out[0], wcs)
    with pytest.raises(ValueError, match="overlaps"):
        pj.spline_prefilter_transpose(m, out=m)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
    assert pj.scatter_cubic(vals, sky, shape, wcs, out=pj.Enmap(out, wcs)).data.data_ptr() == out.data_ptr()
