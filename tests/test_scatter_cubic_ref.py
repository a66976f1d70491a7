"""The yardstick of the order-3 transpose, tests/scatter_cubic_ref.py, against dense solves, the identity B^-T = D B^-1 D^-1,
the adjoint identity with spline_ref (the sampler's yardstick) and one-hot maps; the measurement of KT; and the host-side
argument checks of pj.scatter / pj.scatter_cubic / pj.spline_prefilter_transpose.  No device."""
import re

import numpy as np
import pytest

import scatter_cubic_ref as C
import scatter_ref
import spline_ref as R
from conftest import DEG, ROOT

LD = np.longdouble
SHAPES = [(4, 4), (5, 7), (33, 40)]          # (nx, ny)


def _system(n, cyclic):
    """The system matrix B of one axis: (c[k-1] + 4 c[k] + c[k+1]) / 6 with the cyclic or the whole-sample mirror boundary."""
    B = np.zeros((n, n))
    for k in range(n):
        B[k, k] += 4
        for t in (k - 1, k + 1):
            B[k, int(R.fold(t + 1, n, cyclic)) - 1] += 1
    return B / 6


def _points(nx, ny, n, seed):
    """Pixel positions over the map widened by 1.5 pixels, with x = 0.5, x = nx + 0.5, y = 0.5, y = ny + 0.5 and pixel centres."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, nx + 1.5, n); y = rng.uniform(-0.5, ny + 1.5, n)
    x[:6] = [0.5, nx + 0.5, 1.0, nx, 2.0, 0.5]; y[:6] = [1.5, 2.25, 0.5, ny + 0.5, 3.0, ny + 0.5]
    return x, y


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_transposed_solve_against_dense(nx, ny, periodic):
    g = np.random.default_rng(nx * ny).normal(size=(ny, nx))
    Bx, By = _system(nx, periodic), _system(ny, False)
    if not periodic:
        assert Bx[0, 1] == 2 / 6 and Bx[1, 0] == 1 / 6 and Bx[-1, -2] == 2 / 6 and Bx[-2, -1] == 1 / 6
    dense = np.linalg.solve(By.T, np.linalg.solve(Bx.T, g.T).T)
    got = C.prefilter_transpose(g, periodic)
    assert np.abs(got - dense).max() <= C.bound_t(g, periodic)[0]
    # and it is the transpose of spline_ref's prefilter: <F m, g> = <m, F^T g>
    m = np.random.default_rng(1).normal(size=(ny, nx))
    lhs = np.sum(R.prefilter(m, periodic, LD) * g.astype(LD)); rhs = np.sum(m.astype(LD) * C.prefilter_transpose(g, periodic, LD))
    assert abs(lhs - rhs) <= 64 * R.EPS * np.sum(np.abs(R.prefilter(m, periodic)) * np.abs(g))


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nx,ny", SHAPES + [(80, 40), (360, 181)])
def test_identity_d_prefilter_d_inverse(nx, ny, periodic):
    """What the device runs (spline_ref.prefilter between the two edge scalings) is the direct transposed solve; without D it
    is not, by many orders of magnitude."""
    g = np.random.default_rng(nx + ny).normal(size=(2, ny, nx))
    direct = C.prefilter_transpose(g, periodic)
    via = C.edge_scale(R.prefilter(C.edge_scale(g, periodic, 2.0), periodic), periodic, 0.5)
    assert C.worst_ratio_t(via, direct, g, periodic) <= 1.0
    assert C.worst_ratio_t(R.prefilter(g, periodic), direct, g, periodic) > 1e10


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_adjoint_identity_against_the_samplers_yardstick(nx, ny, periodic):
    """<E F m, d> = <m, F^T E^T d> with E, F from spline_ref and the transposes from this file, dot products in long double;
    F in place of F^T misses by ten orders of magnitude more."""
    x, y = _points(nx, ny, 4000, nx)
    rng = np.random.default_rng(ny)
    m = rng.normal(size=(ny, nx)); d = rng.normal(size=4000)
    pm = R.evaluate_points(R.prefilter(m, periodic), x, y, periodic)
    g = _scatter_pix(x, y, d, nx, ny, periodic)
    scale = float(np.sum(np.abs(pm * d)))
    gap = abs(np.sum(pm.astype(LD) * d.astype(LD)) - np.sum(m.astype(LD) * C.prefilter_transpose(g, periodic).astype(LD)))
    wrong = abs(np.sum(pm.astype(LD) * d.astype(LD)) - np.sum(m.astype(LD) * R.prefilter(g, periodic).astype(LD)))
    print("%d x %d %s: gap %.3g, without D %.3g (of %.3g)" % (nx, ny, "periodic" if periodic else "box", gap / scale, wrong / scale, scale))
    assert gap <= 1e-14 * scale and wrong >= 1e-4 * scale


def _scatter_pix(x, y, d, nx, ny, periodic):
    """E^T from pixel positions (what scatter_cubic_ref.taps does after the oracle's sky2pix)."""
    live = R.in_domain(y, ny) & (np.ones(len(x), bool) if periodic else R.in_domain(x, nx))
    i0, fx = R._split(x[live]); j0, fy = R._split(y[live])
    wx, wy = R.weights(fx), R.weights(fy)
    g = np.zeros(ny * nx)
    for b in range(4):
        for a in range(4):
            np.add.at(g, (R.fold(j0 - 1 + b, ny, False) - 1) * nx + R.fold(i0 - 1 + a, nx, periodic) - 1, (wy[b] * wx[a]) * d[live])
    return g.reshape(ny, nx)


@pytest.mark.parametrize("geom", ["cc_360x181", "box_80x40", "box_4x4", "box_5x7"])
def test_scatter_against_one_hot_maps(pj, O, geom):
    """Tap by tap: <e_p, E^T d> = <E e_p, d> for one-hot coefficient maps e_p, the right side from spline_ref.evaluate_points."""
    shape, wcs = C.geometries(pj)[geom]
    nx, ny = shape
    per = bool(O.is_periodic(wcs, nx))
    sky = scatter_ref.box_points(O, wcs, shape, 3000, 5)
    d = np.random.default_rng(6).normal(size=3000)
    ref, k, S = C.scatter(O, wcs, shape, sky, d)
    pix = O.sky2pix(wcs, shape, sky, safe=True)
    assert np.array_equal(ref[0], _scatter_pix(pix[:, 0], pix[:, 1], d, nx, ny, per))
    rng = np.random.default_rng(7)
    pick = set(rng.integers(0, nx * ny, 12).tolist()) | {0, nx - 1, nx, (ny - 1) * nx, ny * nx - 1, nx + 1}
    for p in sorted(pick):
        e = np.zeros(ny * nx); e[p] = 1.0
        row = R.evaluate_points(e.reshape(ny, nx), pix[:, 0], pix[:, 1], per)
        want = np.sum(row.astype(LD) * d.astype(LD))
        assert abs(ref[0].ravel()[p] - want) <= scatter_ref.bound(k, S)[0].ravel()[p] + 16 * R.EPS * np.sum(np.abs(row * d)), p
    idx, w = C.taps(O, wcs, shape, sky)
    live = idx[:, 0] >= 0
    assert 0 < live.sum() < len(live), "the margin puts points outside the domain"
    assert (idx[~live] == -1).all() and (idx[live] >= 0).all()
    assert np.abs(w[live].sum(axis=1) - 1).max() <= 8 * R.EPS, "the sixteen weights of a point sum to 1"
    assert int(k.sum()) == 16 * int(live.sum())
    if not per:
        assert (np.array([len(set(r)) for r in idx[live]]) < 16).any(), "taps fold onto one pixel next to a mirrored edge"


def test_non_finite_positions_and_values(pj, O):
    shape, wcs = C.geometries(pj)["cc_360x181"]
    sky = scatter_ref.sphere_points(50, 1)
    sky[0, 0] = np.nan; sky[1, 1] = np.inf; sky[2] = [-np.inf, np.nan]
    vals = np.ones(50); vals[10] = np.nan
    idx, w = C.taps(O, wcs, shape, sky)
    assert (idx[:3] == -1).all() and (idx[3:] >= 0).all()
    ref, k, S = C.scatter(O, wcs, shape, sky, vals)
    assert sorted(np.flatnonzero(np.isnan(ref.ravel()))) == sorted(set(idx[10]))
    assert int(k.sum()) == 16 * 47


def test_kt_was_measured(pj, O):
    """KT is 4 x the F^T yardstick's own Float64 error on the GPU tests' inputs, in units of eps * max|plane of D^-1 g|."""
    worst = 0.0
    for name, g, per in C.ft_inputs(pj, O):
        a = C.prefilter_transpose(g, per); b = C.prefilter_transpose(g, per, LD)
        s = np.abs(C.edge_scale(g, per, 2.0)).reshape((-1,) + g.shape[-2:])
        a = a.reshape(s.shape); b = b.reshape(s.shape)
        worst = max(worst, max(float(np.abs(a[i].astype(LD) - b[i]).max() / (C.EPS * s[i].max())) for i in range(len(s))))
    print("F^T yardstick Float64 against long double: %.3f eps max|D^-1 g|; KT = %.2f" % (worst, C.KT))
    assert worst <= C.MEASURED_WORST_FT and C.KT == 4.0 * C.MEASURED_WORST_FT
    assert worst > 0.5 * C.MEASURED_WORST_FT          # and not padded either


# ---- host-side argument checks (no device) ------------------------------------------------------------------------------------
def test_scatter_names_its_limits(pj):
    torch = pytest.importorskip("torch")
    shape, wcs = pj.fullsky_geometry(10.0 * DEG)
    sky = torch.zeros((4, 2), dtype=torch.float64)
    vals = torch.zeros((2, 4), dtype=torch.float64)
    tan = pj.Gnomonic(wcs.cdelt, (10.0, 10.0), (0.0, 0.0))
    for order in (0, 2, 5, "3"):
        with pytest.raises(ValueError, match="order must be 1"):
            pj.scatter(vals, sky, shape, wcs, order=order)
    with pytest.raises(ValueError, match="order=3"):
        pj.scatter(vals, sky, shape, wcs, prefiltered=True)
    for fn in (lambda *a: pj.scatter(*a, order=3), lambda *a: pj.scatter(*a, order=3, prefiltered=True), pj.scatter_cubic):
        with pytest.raises(ValueError, match="CAR only"):
            fn(vals, sky, shape, tan)
        with pytest.raises(ValueError, match="Float64 vals"):
            fn(vals.float(), sky, shape, wcs)
        with pytest.raises(ValueError, match="Float64 skycoords"):
            fn(vals, sky.float(), shape, wcs)
        with pytest.raises(ValueError, match="4 x 4"):
            fn(vals, sky, (36, 3), wcs)
        with pytest.raises(ValueError, match="4 x 4"):
            fn(vals, sky, (3, 19), wcs)
    with pytest.raises(ValueError, match="CAR only"):
        pj.scatter(vals, sky, shape, tan)
    # scatter_bilinear keeps its order of checks: projection and dtype before the shape is read
    with pytest.raises(ValueError, match="CAR only"):
        pj.scatter_bilinear(vals, sky, None, tan)
    with pytest.raises(ValueError, match="Float64 vals"):
        pj.scatter_bilinear(vals.float(), sky, None, wcs)
    with pytest.raises(TypeError):
        pj.spline_prefilter_transpose(torch.zeros((19, 36), dtype=torch.float64))
    with pytest.raises(ValueError, match="Float32"):
        pj.spline_prefilter_transpose(pj.Enmap(torch.zeros((19, 36), dtype=torch.float32), wcs))
    with pytest.raises(ValueError, match="Gnomonic"):
        pj.spline_prefilter_transpose(pj.Enmap(torch.zeros((19, 36), dtype=torch.float64), tan))
    with pytest.raises(ValueError, match="4 x 4"):
        pj.spline_prefilter_transpose(pj.Enmap(torch.zeros((3, 36), dtype=torch.float64), wcs))


def test_header_and_bindings_declare_the_two_entries(pj):
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pixell_hip.h").read(), flags=re.S)
    julia = open(ROOT + "/julia/PixellHIP.jl").read()
    for name in ("pxl_scatter_car_cubic_f64", "pxl_spline_prefilter_transpose_car_f64"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in pj._lib.SIGNATURES
        assert "ccall((:%s, libpixell_hip)" % name in julia, name
    assert re.search(r"function scatter_cubic!\(", julia) and re.search(r"function spline_prefilter_transpose!\(", julia)
    for name in ("scatter", "scatter_cubic", "spline_prefilter_transpose"):
        assert callable(getattr(pj, name))
