"""The yardstick of the polarised pointing matrix, tests/pol_ref.py, against the dense matrix of P_pol and the adjoint identity
<P_pol m, d> = <m, P_pol^T d>; the host-side argument checks of pj.sample_pol / pj.scatter_pol / pj.scatter_pol_weights; and
that header, ctypes table and Julia binding declare the four entries.  No device."""
import re

import numpy as np
import pytest

import pol_ref as P
import scatter_ref
import spline_ref as R
from conftest import DEG, ROOT

LD = np.longdouble
EPS = R.EPS


def _geometry(pj, name):
    if name == "box_6x5":
        shape, wcs = pj.geometry([[3 * DEG, -3 * DEG], [-2.5 * DEG, 2.5 * DEG]], 1.0 * DEG)
        assert shape == (6, 5)
    else:
        shape, wcs = pj.fullsky_geometry(30.0 * DEG)
        assert shape == (12, 7)
    return shape, wcs


def _case(pj, O, name, n=600):
    """Points over the map widened by 1.5 pixels (outside a box, across the seam and the pole rows of the full-circle map), pixel
    centres and edges among them, one position that is not finite; responses from N(0, 1), so q and u are independent."""
    shape, wcs = _geometry(pj, name)
    nx, ny = shape
    rng = np.random.default_rng(nx)
    sky = scatter_ref.box_points(O, wcs, shape, n, 11)
    sky[:4] = O.pix2sky(wcs, np.array([[1.0, 1.0], [nx, ny], [0.5, 2.0], [nx + 0.5, ny + 0.5]]), O.WRAP_NONE)
    sky[4] = [np.nan, 0.1]
    resp = rng.normal(size=(n, 2))
    m = rng.normal(size=(3, ny, nx))
    d = rng.normal(size=n)
    return shape, wcs, sky, resp, m, d


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("name", ["box_6x5", "cc_12x7"])
def test_dense_matrix(pj, O, name, order):
    """P_pol m, P_pol^T d and the weights planes against the dense matrix built tap by tap, each within a few roundings of
    sum |A| |x| (and the scatter's own k * 2^-52 * S)."""
    shape, wcs, sky, resp, m, d = _case(pj, O, name)
    nx, ny = shape
    npix = nx * ny
    per = bool(O.is_periodic(wcs, nx))
    assert per == (name == "cc_12x7")
    A = P.dense(O, wcs, shape, sky, resp, order)
    live = np.abs(A[:, :npix]).sum(axis=1) > 0
    assert not live[4] and 0.5 < live.mean() < 1.0, "some points are on the map, the one that is not finite is not"
    # the weights of a point sum to 1 (order 3: every live point; order 1: unless a tap is dropped), and the Q and U blocks
    # carry q and u times as much
    rows = A[:, :npix].sum(axis=1)
    assert rows.max() <= 1 + 8 * EPS and np.abs(rows - 1).min() <= 8 * EPS
    if order == 3:
        assert np.abs(rows[live] - 1).max() <= 8 * EPS
    for c in (1, 2):
        assert np.abs(A[:, c * npix:(c + 1) * npix].sum(axis=1) - resp[:, c - 1] * rows).max() <= 16 * EPS * np.abs(resp).max()
    # forward
    got = P.sample(O, wcs, shape, m, sky, resp, order, prefiltered=True)
    assert np.isnan(got[4]) and np.isfinite(np.delete(got, 4)).all()
    want = A @ m.ravel()
    tol = 16 * EPS * (np.abs(A) @ np.abs(m.ravel()))
    ok = np.arange(len(got)) != 4
    assert np.all(np.abs(got - want)[ok] <= tol[ok])
    assert np.all(got[ok & ~live] == 0.0)
    if order == 3:
        full = P.sample(O, wcs, shape, m, sky, resp, 3)
        c = R.prefilter(m, per)
        assert np.all(np.abs(full - A @ c.ravel())[ok] <= (16 * EPS * (np.abs(A) @ np.abs(c.ravel())))[ok])
        assert np.abs(full - got)[ok].max() > 1e-3, "the prefilter is part of P_pol at order 3"
    # transpose, signal
    ref, k, S = P.scatter(O, wcs, shape, sky, d, resp, order)
    assert ref.shape == (3, ny, nx)
    want = (A.T @ d).reshape(3, ny, nx)
    tol = scatter_ref.bound(k, S) + 16 * EPS * (np.abs(A).T @ np.abs(d)).reshape(3, ny, nx)
    assert np.all(np.abs(ref - want) <= tol)
    # weights: P^T applied to the six products, through the I block of the matrix
    t6 = P.terms(d, resp, 1)
    q, u = resp[:, 0], resp[:, 1]
    exact = np.stack([d, q * d, u * d, q * q * d, q * u * d, u * u * d])
    assert np.abs(t6 - exact).max() <= 4 * EPS * np.abs(exact).max()
    refw, kw, Sw = P.scatter(O, wcs, shape, sky, d, resp, order, mode=1)
    assert refw.shape == (6, ny, nx)
    assert np.array_equal(refw[:3].view(np.int64), ref.view(np.int64)), "the first three weight planes are the signal's"
    B = A[:, :npix]
    for c in range(6):
        tol = scatter_ref.bound(kw[c], Sw[c]) + 16 * EPS * (np.abs(B).T @ np.abs(t6[c])).reshape(ny, nx)
        assert np.all(np.abs(refw[c] - (B.T @ t6[c]).reshape(ny, nx)) <= tol), c
    # an initial map is a term of its own, and nonzero_terms counts what the scatter adds
    nz = P.nonzero_terms(O, wcs, shape, sky, d, resp, order)
    assert nz.shape == k.shape and np.all(nz <= k) and nz.sum() > 0


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("name", ["box_6x5", "cc_12x7"])
def test_adjoint_identity(pj, O, name, order):
    """<P_pol m, d> = <m, P_pol^T d>, dot products in long double, within the 1e-14 * scale of
    tests/test_scatter_cubic_ref.py's scalar identity; three times as many terms enter the scale,
    sum_k |d_k| (|s_I| + |q s_Q| + |u s_U|).  At order 3 P_pol = E_pol F and P_pol^T = F^T E_pol^T."""
    shape, wcs, sky, resp, m, d = _case(pj, O, name, n=4000)
    keep = np.arange(len(d)) != 4                                   # the position that is not finite: NaN forward, nothing back
    s = P.sample_planes(O, wcs, shape, m, sky, order)
    pm = P.combine(s, resp)
    assert np.isnan(pm[4])
    ptd, g, k, S = P.scatter_full(O, wcs, shape, sky, d, resp, order)
    assert np.isfinite(ptd).all()
    scale = float(np.sum(np.abs(d[keep]) * (np.abs(s[0]) + np.abs(resp[:, 0] * s[1]) + np.abs(resp[:, 1] * s[2]))[keep]))
    gap = float(abs(np.sum(pm[keep].astype(LD) * d[keep].astype(LD)) - np.sum(m.astype(LD) * ptd.astype(LD))))
    print("%s order %d: gap %.3g of %.3g" % (name, order, gap, scale))
    assert scale > 0 and gap <= 1e-14 * scale
    if order == 3:
        wrong = R.prefilter(g, bool(O.is_periodic(wcs, shape[0])))
        miss = float(abs(np.sum(pm[keep].astype(LD) * d[keep].astype(LD)) - np.sum(m.astype(LD) * wrong.astype(LD))))
        assert miss >= 1e-4 * scale, "the untransposed prefilter passes: the test shows nothing"
    # dropping a response changes the answer: the identity is not the scalar one in disguise
    flat = P.combine(s, np.zeros_like(resp))
    assert float(abs(np.sum(flat[keep].astype(LD) * d[keep].astype(LD)) - np.sum(m.astype(LD) * ptd.astype(LD)))) > 1e-6 * scale


def test_rows_windows_and_empty_batches(pj, O):
    """The order-1 yardstick on a declination strip is the strip of the whole map's, and n = 0 gives empty results."""
    shape, wcs, sky, resp, m, d = _case(pj, O, "cc_12x7")
    whole, k, S = P.scatter(O, wcs, shape, sky, d, resp)
    part, kp, Sp = P.scatter(O, wcs, shape, sky, d, resp, row0=2, nrows=3)
    assert part.shape == (3, 3, 12) and np.all(np.abs(part - whole[:, 2:5]) <= scatter_ref.bound(k, S)[:, 2:5])
    a = P.sample(O, wcs, shape, np.ascontiguousarray(m[:, 2:5]), sky, resp, row0=2, nrows=3)
    z = m.copy(); z[:, :2] = 0; z[:, 5:] = 0
    b = P.sample(O, wcs, shape, z, sky, resp)
    ok = np.arange(len(a)) != 4
    assert np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64)), "rows outside the window read as zero"
    ref, k0, S0 = P.scatter(O, wcs, shape, np.zeros((0, 2)), np.zeros(0), np.zeros((0, 2)), mode=1)
    assert ref.shape == (6, 7, 12) and not ref.any() and not k0.any()


# ---- host-side argument checks (no device) ------------------------------------------------------------------------------------
def test_pol_calls_name_their_limits(pj):
    torch = pytest.importorskip("torch")
    shape, wcs = pj.fullsky_geometry(10.0 * DEG)
    sky = torch.zeros((4, 2), dtype=torch.float64)
    resp = torch.zeros((4, 2), dtype=torch.float64)
    vals = torch.zeros(4, dtype=torch.float64)
    tan = pj.Gnomonic(wcs.cdelt, (10.0, 10.0), (0.0, 0.0))
    m = pj.Enmap(torch.zeros((3, 19, 36), dtype=torch.float64), wcs)
    for fn in (pj.scatter_pol, pj.scatter_pol_weights):
        for order in (0, 2, "3"):
            with pytest.raises(ValueError, match="order must be 1"):
                fn(vals, sky, resp, shape, wcs, order=order)
        with pytest.raises(ValueError, match="order=3"):
            fn(vals, sky, resp, shape, wcs, prefiltered=True)
        with pytest.raises(ValueError, match="order=1 only"):
            fn(vals, sky, resp, shape, wcs, order=3, src_rows=(0, 19), full_shape=shape)
        with pytest.raises(ValueError, match="4 x 4"):
            fn(vals, sky, resp, (36, 3), wcs, order=3)
        with pytest.raises(ValueError, match="CAR only"):
            fn(vals, sky, resp, shape, tan)
        with pytest.raises(ValueError, match="Float64 vals"):
            fn(vals.float(), sky, resp, shape, wcs)
        with pytest.raises(ValueError, match="Float64 skycoords"):
            fn(vals, sky.float(), resp, shape, wcs)
    for order in (0, 2, "3"):
        with pytest.raises(ValueError, match="order must be 1"):
            pj.sample_pol(m, sky, resp, order=order)
    with pytest.raises(ValueError, match="order=3"):
        pj.sample_pol(m, sky, resp, prefiltered=True)
    with pytest.raises(ValueError, match="order=1 only"):
        pj.sample_pol(m, sky, resp, order=3, src_rows=(0, 19), full_shape=shape)
    with pytest.raises(TypeError):
        pj.sample_pol(m.data, sky, resp)
    for bad in (torch.zeros((2, 19, 36), dtype=torch.float64), torch.zeros((19, 36), dtype=torch.float64),
                torch.zeros((6, 19, 36), dtype=torch.float64)):
        with pytest.raises(ValueError, match="three components"):
            pj.sample_pol(pj.Enmap(bad, wcs), sky, resp)
    with pytest.raises(ValueError, match="Float64|Float32"):
        pj.sample_pol(pj.Enmap(m.data.float(), wcs), sky, resp)
    with pytest.raises(ValueError, match="Float64|Float32"):
        pj.sample_pol(pj.Enmap(m.data.float(), wcs), sky, resp, order=3)
    with pytest.raises(ValueError, match="CAR only|Gnomonic"):
        pj.sample_pol(pj.Enmap(m.data, tan), sky, resp)
    with pytest.raises(ValueError, match="4 x 4"):
        pj.sample_pol(pj.Enmap(torch.zeros((3, 3, 36), dtype=torch.float64), wcs), sky, resp, order=3)


def test_header_and_bindings_declare_the_four_entries(pj):
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pixell_hip.h").read(), flags=re.S)
    julia = open(ROOT + "/julia/PixellHIP.jl").read()
    for name in ("pxl_sample_car_pol_bilinear_f64", "pxl_sample_car_pol_cubic_f64", "pxl_scatter_car_pol_bilinear_f64",
                 "pxl_scatter_car_pol_cubic_f64"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in pj._lib.SIGNATURES
        assert "ccall((:%s, libpixell_hip)" % name in julia, name
        assert hasattr(pj.load_library(), name)
    exports = " ".join(re.findall(r"^export (.*)$", julia, flags=re.M)).replace(",", " ").split()
    for fn in ("sample_pol", "scatter_pol!", "scatter_pol_weights!"):
        assert fn in exports, fn
    assert re.search(r"function sample_pol\(", julia) and re.search(r"^scatter_pol!\(", julia, flags=re.M)
    for name in ("sample_pol", "scatter_pol", "scatter_pol_weights"):
        assert callable(getattr(pj, name))
