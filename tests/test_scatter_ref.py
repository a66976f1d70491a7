"""The scatter-add yardstick (tests/scatter_ref.py) held to the oracle's forward sampler, CPU only.

1. Adjoint identity <P m, d> = <m, P^T d> with P m from oracle.sample_bilinear, on the 360 x 181 full sky, the 80 x 40 box and a
   strip window of the full sky, within 2^-53 * sum_p |m_p| S_p (8 + 2 k_p), both dot products in longdouble.
2. Tap by tap: on maps that are 1 at one pixel, the oracle's sample of point k IS the weight with which k reaches that pixel
   (the lerps multiply by 1 and add 0 exactly), so the whole response matrix of the oracle must equal the yardstick's taps --
   every tap the yardstick drops is one the oracle reads as 0, and no tap the oracle reads is missing.
3. The product's side of the interface that needs no GPU: the symbol, its signature and the Python entry exist."""
import ctypes

import numpy as np
import pytest

import scatter_ref as R
from conftest import DEG


def _edge_points(O, wcs, shape, seed):
    """Random points over the map widened by 1.5 pixels, plus points on the pixel centres and half a pixel beyond every edge
    and corner, and (on the full sky) the poles and both sides of the seam."""
    nx, ny = shape
    pts = [R.box_points(O, wcs, shape, 1500, seed)]
    xs = np.array([0.25, 0.5, 0.75, 1.0, 1.5, nx - 0.5, nx, nx + 0.25, nx + 0.5, nx + 0.75, nx + 1.0, nx / 2 + 0.3])
    ys = np.array([0.25, 0.5, 0.75, 1.0, 1.5, ny - 0.5, ny, ny + 0.25, ny + 0.5, ny + 0.75, ny + 1.0, ny / 2 + 0.3])
    gx, gy = np.meshgrid(xs, ys)
    pts.append(O.pix2sky(wcs, np.stack([gx.ravel(), gy.ravel()], axis=1), O.WRAP_NONE))
    pts.append(np.array([[0.3, np.pi / 2], [-2.0, -np.pi / 2], [np.pi, 0.1], [-np.pi, 0.1], [np.nextafter(np.pi, 0), -0.2], [3 * np.pi + 0.01, 0.4]]))
    return np.concatenate(pts)


ADJOINT_CASES = {"cc_360x181": ("cc_360x181", None), "box_80x40": ("box_80x40", None), "strip_of_cc_360x181": ("cc_360x181", (60, 50))}


@pytest.mark.parametrize("case", sorted(ADJOINT_CASES))
def test_adjoint_identity_against_the_oracle(pj, O, case):
    geom, window = ADJOINT_CASES[case]
    shape, wcs = R.geometries(pj)[geom]
    row0, nrows = window if window else (0, shape[1])
    rng = np.random.default_rng(len(case))
    sky = np.concatenate([R.sphere_points(20000, 5), _edge_points(O, wcs, shape, 6)])
    m = rng.normal(size=(2, nrows, shape[0]))
    d = rng.normal(size=(2, sky.shape[0]))
    pm = O.sample_bilinear(wcs, (shape[0], shape[1], 2), m, sky, src_row0=row0, src_nrows=nrows)
    assert np.isfinite(pm).all()
    ref, k, S = R.scatter(O, wcs, shape, sky, d, row0=row0, nrows=nrows)
    idx, _w = R.taps(O, wcs, shape, sky, row0, nrows)
    assert (idx < 0).any() and (idx >= 0).any(), "the case must drop some taps and keep some"
    gap, b = R.adjoint_gap(m, pm, d, ref, k, S)
    print("%s: |<Pm,d> - <m,PTd>| = %.3g, bound %.3g, %d of %d taps dropped" % (case, gap, b, int((idx < 0).sum()), idx.size))
    assert b > 0 and gap <= b


def _small_geometries(pj):
    g = {"periodic_24x13": (pj.fullsky_geometry(15.0 * DEG), None),
         "box_12x8": (pj.geometry([[12 * DEG, -12 * DEG], [-8 * DEG, 8 * DEG]], 2.0 * DEG), None),
         "strip_of_periodic_24x13": (pj.fullsky_geometry(15.0 * DEG), (4, 5)),
         "empty_window": (pj.fullsky_geometry(15.0 * DEG), (6, 0))}
    return g


@pytest.mark.parametrize("case", ["periodic_24x13", "box_12x8", "strip_of_periodic_24x13"])
def test_every_tap_is_the_oracles(pj, O, case):
    (shape, wcs), window = _small_geometries(pj)[case]
    nx, ny = shape
    row0, nrows = window if window else (0, ny)
    sky = _edge_points(O, wcs, shape, 11)
    n, npix = sky.shape[0], nrows * nx
    onehot = np.eye(npix).reshape(npix, nrows, nx)                     # component p is 1 at pixel p
    G = O.sample_bilinear(wcs, (nx, ny, npix), onehot, sky, src_row0=row0, src_nrows=nrows)        # (npix, n)
    idx, w = R.taps(O, wcs, shape, sky, row0, nrows)
    W = np.zeros((npix, n))
    for t in range(4):
        on = idx[:, t] >= 0
        np.add.at(W, (idx[on, t], np.nonzero(on)[0]), w[on, t])
    # a point reaches a pixel through at most one tap on these maps (nx > 2), so W holds single weights, not sums
    assert np.array_equal(G, W), "%d entries of the response matrix differ" % int((G != W).sum())
    dropped = idx < 0
    assert dropped.any() and not dropped.all()
    assert (dropped.sum(axis=1) == 4).any() and ((dropped.sum(axis=1) > 0) & (dropped.sum(axis=1) < 4)).any(), \
        "need points wholly off the map and points with some taps off it"
    if wcs is not None and O.is_periodic(wcs, nx):
        cols = idx % nx
        seam = ((cols[:, 0] == nx - 1) & (cols[:, 1] == 0) & (idx[:, 0] >= 0) & (idx[:, 1] >= 0))
        assert seam.any(), "no cell straddles the seam"


def test_non_finite_points_and_empty_window(pj, O):
    (shape, wcs), _ = _small_geometries(pj)["periodic_24x13"]
    sky = np.array([[0.1, 0.2], [np.nan, 0.2], [0.1, np.inf], [-np.inf, np.nan], [1.0, -0.4]])
    pm = O.sample_bilinear(wcs, (shape[0], shape[1], 1), np.ones((1, shape[1], shape[0])), sky)
    idx, _w = R.taps(O, wcs, shape, sky)
    assert np.array_equal(np.isnan(pm[0]), (idx < 0).all(axis=1)) and np.isnan(pm[0]).sum() == 3
    out0 = np.full((1, shape[1], shape[0]), 0.5)
    ref, k, S = R.scatter(O, wcs, shape, sky, np.ones(5), out=out0)
    assert k.sum() == out0.size + 8 and np.isfinite(ref).all()
    (shape, wcs), (row0, nrows) = _small_geometries(pj)["empty_window"]
    ref, k, S = R.scatter(O, wcs, shape, sky, np.ones(5), row0=row0, nrows=nrows)
    assert ref.shape == (1, 0, shape[0])


def test_bound_is_k_2m52_S():
    k, S = np.array([0, 1, 5]), np.array([0.0, 2.0, 3.0])
    assert np.array_equal(R.bound(k, S), [0.0, 2.0 ** -51, 15 * 2.0 ** -52])


def test_product_declares_the_transpose(pj):
    """The device counterpart of the yardstick: exported by the library, bound with the sampler's argument layout, public."""
    lib = ctypes.CDLL(pj.library_path())
    assert hasattr(lib, "pxl_scatter_car_bilinear_f64")
    assert pj._lib.SIGNATURES["pxl_scatter_car_bilinear_f64"] == pj._lib.SIGNATURES["pxl_sample_car_bilinear_f64"]
    assert callable(pj.scatter_bilinear)
    # argument checks run before any HIP call
    lib = pj.load_library()
    assert lib.pxl_scatter_car_bilinear_f64(None, None, None, 0, 0, 0, None, None, None) == -22
    shape, wcs = pj.fullsky_geometry(1.0 * DEG)
    w = wcs.to_struct()
    shp = pj._lib.shape_arr((360, 181, 1))
    assert lib.pxl_scatter_car_bilinear_f64(ctypes.byref(w), shp, None, 0, 181, 0, None, None, None) == 0            # n = 0
    assert lib.pxl_scatter_car_bilinear_f64(ctypes.byref(w), shp, None, 0, 181, -1, None, None, None) == -22
    assert lib.pxl_scatter_car_bilinear_f64(ctypes.byref(w), shp, None, 100, 82, 0, None, None, None) == -22
    assert "window" in pj._lib.last_error()
    assert lib.pxl_scatter_car_bilinear_f64(ctypes.byref(w), pj._lib.shape_arr((360, 181, 0)), None, 0, 181, 0, None, None, None) == -22
    assert lib.pxl_scatter_car_bilinear_f64(ctypes.byref(w), shp, None, 0, 181, 4, None, None, None) == -22          # null with n > 0
