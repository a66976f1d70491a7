"""The order-0 yardstick tests/nearest_ref.py held to independent definitions, and the host side of the order-0 operators
(DESIGN.md 4.15).  CPU only: nothing here touches the device."""
import re

import numpy as np
import pytest

import nearest_ref as N
import pol_ref
import polsolve_ref
import scatter_ref as R
from conftest import DEG, ROOT

LD = np.longdouble
SMALL = ("box_5x7", "box_2x2", "box_1x1")


def _inputs(pj, O, geom, n, seed):
    shape, wcs = N.geometries(pj)[geom]
    sky = N.points(O, wcs, shape, n, seed)
    rng = np.random.default_rng(seed + 5)
    return shape, wcs, sky, rng.normal(size=(n, 2)), rng.normal(size=(3, shape[1], shape[0])), rng.normal(size=n)


# ---- the yardstick against its dense matrix --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", SMALL + ("box_80x40",))
def test_against_the_dense_matrix(pj, O, geom):
    """sample() is the one-hot matrix times the map exactly (one term per row), scatter() its transpose times the values within the
    summation bound, for the scalar and the polarised forms; a point without a pixel has a zero row."""
    n = 3000 if geom == "box_80x40" else 600
    shape, wcs, sky, resp, m, d = _inputs(pj, O, geom, n, 11)
    fin = np.isfinite(sky).all(axis=1)
    A = N.dense(O, wcs, shape, sky)
    s = N.sample(O, wcs, shape, m, sky)
    assert np.array_equal(np.isnan(s[0]), ~fin)
    for c in range(3):
        assert np.array_equal((A @ m[c].ravel())[fin], s[c][fin])
    ref, k, S = N.scatter(O, wcs, shape, sky, np.stack([d, 2 * d]))
    assert np.all(np.abs(ref[0].ravel() - A.T @ d) <= R.bound(k, S)[0].ravel())
    assert np.array_equal(k[0].ravel(), A.sum(axis=0).astype(np.int64)) and int(k[0].sum()) == int((N.taps(O, wcs, shape, sky)[0] >= 0).sum())
    Ap = N.dense(O, wcs, shape, sky, resp)
    sp = N.sample_pol(O, wcs, shape, m, sky, resp)
    exact = Ap.astype(LD) @ m.ravel().astype(LD)
    tol = 2.0 ** -53 * 5 * (np.abs(s[0]) + np.abs(resp[:, 0] * s[1]) + np.abs(resp[:, 1] * s[2]))
    assert np.all(np.abs(sp[fin] - exact[fin]) <= tol[fin])
    for mode, planes in ((0, 3), (1, 6)):
        rp, kp, Sp = N.scatter_pol(O, wcs, shape, sky, d, resp, mode)
        assert rp.shape == (planes, shape[1], shape[0])
    rp, kp, Sp = N.scatter_pol(O, wcs, shape, sky, d, resp)
    want = (Ap.T.astype(LD) @ d.astype(LD)).reshape(rp.shape)
    assert np.all(np.abs(rp - want) <= (kp + 1) * 2.0 ** -53 * Sp * 2)
    assert (k > 1).any() and (N.taps(O, wcs, shape, sky)[0] < 0).any()


@pytest.mark.parametrize("geom", N.GEOMS)
def test_adjoint_identity(pj, O, geom):
    """<P m, d> = <m, P^T d> within the summation bound, scalar and polarised, points without a pixel and all."""
    shape, wcs, sky, resp, m, d = _inputs(pj, O, geom, 4000, 13)
    keep = np.isfinite(sky).all(axis=1)
    s = N.sample(O, wcs, shape, m, sky)
    ref, k, S = N.scatter(O, wcs, shape, sky, np.stack([d, d, d]))
    gap, b = N.adjoint_gap(m, s[:, keep], d[keep], ref, k, S)
    print("%s: scalar adjoint gap %.3g, bound %.3g" % (geom, gap, b))
    assert gap <= b
    sp = N.sample_pol(O, wcs, shape, m, sky, resp)
    rp, kp, Sp = N.scatter_pol(O, wcs, shape, sky, d, resp)
    gap, b = N.adjoint_gap_pol(m, sp[keep], d[keep], rp, kp, Sp, s[:, keep], resp[keep])
    print("%s: polarised adjoint gap %.3g, bound %.3g" % (geom, gap, b))
    assert gap <= b
    scale = float(np.sum(np.abs(sp[keep] * d[keep])))
    flat = pol_ref.combine(s[:, keep], np.zeros_like(resp[keep]))
    if geom != "box_1x1":
        assert abs(float(np.sum(flat.astype(LD) * d[keep].astype(LD)) - np.sum(m.astype(LD) * rp.astype(LD)))) > 1e-6 * scale


# ---- against the bilinear taps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", N.GEOMS)
def test_the_pixel_is_the_heaviest_bilinear_tap(pj, O, geom):
    """The nearest pixel is the tap (a, b) = (fx >= 0.5, fy >= 0.5) of scatter_ref.taps' four, index for index (dropped where it is
    dropped), that tap's weight is the largest of the four and at least 0.25."""
    shape, wcs = N.geometries(pj)[geom]
    sky = N.points(O, wcs, shape, 6000, 17)
    sky = sky[np.isfinite(sky).all(axis=1)]
    idx, fin, _i, _j, fx, fy = N.cells(O, wcs, shape, sky)
    tidx, tw = R.taps(O, wcs, shape, sky)
    t = (fx >= 0.5).astype(int) + 2 * (fy >= 0.5).astype(int)
    rows = np.arange(len(sky))
    assert np.array_equal(tidx[rows, t], idx)
    assert np.array_equal(tw[rows, t], tw.max(axis=1)) and float(tw[rows, t].min()) >= 0.25
    cx, cy = N.classes(O, wcs, shape, sky)
    assert (cx == 0).sum() >= 9 and (cy == 0).sum() >= 9 and (idx >= 0).any() and (idx < 0).any()


def test_ties_go_up_at_the_seam_and_the_pole_rows(pj, O):
    """Every x = i + 0.5, y = j + 0.5 round-trips through pix2sky and sky2pix to a fraction of exactly 0.5 (full sky and boxes),
    and lands on pixel (i + 1, j + 1): x = nx + 0.5 is column 1 of the periodic map and off a box, y = 0.5 is row 1,
    y = ny + 0.5 is off the map.  Moved by 2^-30 pixel either way the points leave the tie on the side they were moved to."""
    for geom in N.GEOMS:
        shape, wcs = N.geometries(pj)[geom]
        nx, ny = shape
        sky = N.edge_points(O, wcs, shape)
        cx, cy = N.classes(O, wcs, shape, sky)
        assert not cx.any() and not cy.any(), "%s: an edge point does not round-trip to a fraction of 0.5" % geom
        idx, _fin, i, j, _fx, _fy = N.cells(O, wcs, shape, sky)
        wi, wj = np.meshgrid(np.arange(-1, nx + 2) + 1, np.arange(-1, ny + 2) + 1, indexing="xy")
        per = bool(O.is_periodic(wcs, nx))
        assert np.array_equal(j, wj.ravel())
        assert not ((i - wi.ravel()) % nx).any() if per else np.array_equal(i, wi.ravel())      # safe=True brings RA back by whole turns
        on = (wj.ravel() >= 1) & (wj.ravel() <= ny) & (per | ((wi.ravel() >= 1) & (wi.ravel() <= nx)))
        col = (wi.ravel() - 1) % nx if per else wi.ravel() - 1
        assert np.array_equal(idx, np.where(on, (wj.ravel() - 1) * nx + col, -1))
        for shift, cls in ((-N.NUDGE, -1), (N.NUDGE, 1)):
            cx, cy = N.classes(O, wcs, shape, N.edge_points(O, wcs, shape, shift))
            assert np.all(cx == cls) and np.all(cy == cls)


def test_against_scipy_map_coordinates(pj, O):
    """scipy.ndimage.map_coordinates(order=0) picks the same pixel wherever the point is not on a tie: grid-wrap along RA on the
    periodic map (rows on the map only), grid-constant 0 on the boxes."""
    ndi = pytest.importorskip("scipy.ndimage")
    for geom in N.GEOMS:
        shape, wcs = N.geometries(pj)[geom]
        nx, ny = shape
        sky = N.points(O, wcs, shape, 6000, 19)
        sky = sky[np.isfinite(sky).all(axis=1)]
        cx, cy = N.classes(O, wcs, shape, sky)
        sky = sky[(cx != 0) & (cy != 0)]
        m = np.random.default_rng(3).normal(size=(ny, nx))
        pix = O.sky2pix(wcs, (nx, ny), sky, safe=True)
        got = N.sample(O, wcs, shape, m, sky)[0]
        if O.is_periodic(wcs, nx):
            rows = (pix[:, 1] > 0.5) & (pix[:, 1] < ny + 0.5)
            want = ndi.map_coordinates(m, [pix[rows, 1] - 1, pix[rows, 0] - 1], order=0, mode="grid-wrap")
            assert np.array_equal(got[rows], want) and not got[~rows].any() and (~rows).any()
        else:
            want = ndi.map_coordinates(m, [pix[:, 1] - 1, pix[:, 0] - 1], order=0, mode="grid-constant", cval=0.0)
            assert np.array_equal(got, want)
        assert len(sky) > 4000


def test_row_windows_and_empty_batches(pj, O):
    shape, wcs, sky, resp, m, d = _inputs(pj, O, "cc_360x181", 5000, 23)
    whole, k, S = N.scatter_pol(O, wcs, shape, sky, d, resp)
    part, kp, Sp = N.scatter_pol(O, wcs, shape, sky, d, resp, row0=60, nrows=50)
    assert part.shape == (3, 50, 360) and np.array_equal(part, whole[:, 60:110]) and np.array_equal(kp, k[:, 60:110])
    a = N.sample(O, wcs, shape, np.ascontiguousarray(m[:, 60:110]), sky, row0=60, nrows=50)
    z = m.copy(); z[:, :60] = 0; z[:, 110:] = 0
    assert np.array_equal(a.view(np.int64), N.sample(O, wcs, shape, z, sky).view(np.int64))
    (r, kr, _), (w6, k6, _) = N.bin(O, wcs, shape, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0), np.zeros(0))
    assert r.shape == (3, 181, 360) and w6.shape == (6, 181, 360) and not r.any() and not kr.any() and not k6.any()


# ---- the map: the numpy recipe inside the bound the device is held to ------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["box_5x7", "box_80x40", "cc_360x181"])
def test_the_numpy_map_recovers_the_sky_within_the_bound(pj, O, geom):
    """nearest_ref.bin + polsolve_ref.solve of noiseless d = P m0 returns m0 on every solved pixel within
    16 (k + 50) 2^-52 ||m0(p)||_1 / rc(p) (nearest_ref.map_bound), and the order-1 pixel blocks would not: on the boxes the bilinear
    binned map of the same samples misses m0 by more than 0.1."""
    c = N.map_case(pj, O, geom)
    s = c.solved
    assert np.array_equal(np.flatnonzero(c.hits.ravel() == 0), c.unhit) and not c.solved[c.hits < 3].any()
    assert s[c.hits > 0].mean() >= (0.95 if geom == "cc_360x181" else 1.0)
    err = np.abs(c.map - c.m0).max(axis=0)
    b = N.map_bound(c.m0, c.hits, c.rcond)
    print("%s: worst error / bound = %.3g on %d solved pixels, worst error %.3g, min rcond %.3g, mean hits %.1f" % (
        geom, float((err[s] / b[s]).max()), int(s.sum()), float(err[s].max()), float(c.rcond[s].min()), float(c.hits.mean())))
    assert np.all(err[s] <= b[s])
    assert not c.map[:, ~s].view(np.int64).any() and not c.rcond[c.hits == 0].view(np.int64).any()
    if geom == "cc_360x181":
        return
    rhs1 = pol_ref.scatter(O, c.wcs, c.shape, c.sky, c.w * c.d, c.resp)[0]
    w1 = pol_ref.scatter(O, c.wcs, c.shape, c.sky, c.w, c.resp, mode=1)[0]
    x1, _rc1, info1 = polsolve_ref.solve(w1.reshape(6, -1), rhs1.reshape(3, -1), N.RCOND_MIN)
    miss = np.abs(x1.reshape(c.m0.shape) - c.m0).max(axis=0)[info1["ok"].reshape(s.shape)].max()
    print("%s: the order-1 binned map of the same samples misses m0 by %.3g" % (geom, float(miss)))
    assert miss > 0.1


@pytest.mark.parametrize("geom", ["box_5x7", "box_80x40"])
def test_the_normal_operator_is_the_blocks(pj, O, geom):
    """scatter_pol(w * sample_pol(x)) against polsolve_ref.apply(weights, x) per pixel within nearest_ref.blocks_bound, and the
    bound is not slack by orders of magnitude."""
    c = N.map_case(pj, O, geom)
    x = np.random.default_rng(5).normal(size=c.m0.shape)
    comp = N.scatter_pol(O, c.wcs, c.shape, c.sky, c.w * N.sample_pol(O, c.wcs, c.shape, x, c.sky, c.resp), c.resp)[0]
    blk = polsolve_ref.apply(c.w6.reshape(6, -1), x.reshape(3, -1)).reshape(comp.shape)
    b = N.blocks_bound(O, c.wcs, c.shape, x, c.sky, c.resp, c.w)
    ratio = float((np.abs(comp - blk)[b > 0] / b[b > 0]).max())
    print("%s: composition against the blocks, worst gap / bound = %.3g" % (geom, ratio))
    assert np.all(np.abs(comp - blk) <= b) and ratio > 1e-4 and (b[:, c.hits > 0] > 0).all()


# ---- host-side argument checks (no device) -----------------------------------------------------------------------------------------
def test_order_zero_is_still_refused_by_the_order_argument(pj):
    torch = pytest.importorskip("torch")
    shape, wcs = pj.fullsky_geometry(10.0 * DEG)
    m = pj.Enmap(torch.zeros((3, 19, 36), dtype=torch.float64), wcs)
    sky = torch.zeros((4, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="order must be 1"):
        pj.sample(m, None, order=0)
    with pytest.raises(ValueError, match="order must be 1"):
        pj.scatter(torch.zeros(4, dtype=torch.float64), sky, shape, wcs, order=0)
    with pytest.raises(TypeError):
        pj.binned_map_pol(torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), sky, sky, shape, wcs, order=0)


def test_nearest_calls_name_their_limits(pj):
    """Every new function refuses CPU tensors (there is no CPU fallback), Gnomonic maps and Float32 with a message that says so,
    and wrong shapes, before anything reaches the library."""
    torch = pytest.importorskip("torch")
    shape, wcs = pj.fullsky_geometry(10.0 * DEG)
    f64 = dict(dtype=torch.float64)
    sky, resp, vals = torch.zeros((4, 2), **f64), torch.zeros((4, 2), **f64), torch.zeros(4, **f64)
    tan = pj.Gnomonic(wcs.cdelt, (10.0, 10.0), (0.0, 0.0))
    m = pj.Enmap(torch.zeros((3, 19, 36), **f64), wcs)
    calls = {
        "sample_nearest": lambda **k: pj.sample_nearest(k.get("m", m), k.get("sky", sky)),
        "scatter_nearest": lambda **k: pj.scatter_nearest(k.get("vals", vals), k.get("sky", sky), shape, k.get("wcs", wcs)),
        "sample_pol_nearest": lambda **k: pj.sample_pol_nearest(k.get("m", m), k.get("sky", sky), k.get("resp", resp)),
        "scatter_pol_nearest": lambda **k: pj.scatter_pol_nearest(k.get("vals", vals), k.get("sky", sky), k.get("resp", resp), shape, k.get("wcs", wcs)),
        "scatter_pol_weights_nearest": lambda **k: pj.scatter_pol_weights_nearest(k.get("vals", vals), k.get("sky", sky), k.get("resp", resp), shape, k.get("wcs", wcs)),
        "bin_pol_nearest": lambda **k: pj.bin_pol_nearest(k.get("vals", vals), k.get("w", vals), k.get("sky", sky), k.get("resp", resp), shape, k.get("wcs", wcs)),
        "binned_map_pol_nearest": lambda **k: pj.binned_map_pol_nearest([(k.get("vals", vals), k.get("w", vals), k.get("sky", sky), k.get("resp", resp))], shape, k.get("wcs", wcs)),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()
        with pytest.raises(ValueError, match="CAR only"):
            call(wcs=tan, m=pj.Enmap(m.data, tan))
        with pytest.raises(ValueError, match="Float64 skycoords"):
            call(sky=sky.float())
        with pytest.raises(ValueError, match="Float64"):
            call(vals=vals.float(), m=pj.Enmap(m.data.float(), wcs))
        if "pol" in name:
            with pytest.raises(ValueError, match="Float64 resp"):
                call(resp=resp.float())
    for fn in (pj.sample_nearest, pj.sample_pol_nearest):
        with pytest.raises(TypeError, match="takes an Enmap"):
            fn(m.data, sky, *([resp] if fn is pj.sample_pol_nearest else []))
    for bad in (torch.zeros((2, 19, 36), **f64), torch.zeros((19, 36), **f64), torch.zeros((6, 19, 36), **f64)):
        with pytest.raises(ValueError, match="three components"):
            pj.sample_pol_nearest(pj.Enmap(bad, wcs), sky, resp)
    with pytest.raises(ValueError, match="at least one batch"):
        pj.binned_map_pol_nearest([], shape, wcs)
    with pytest.raises(ValueError, match="a batch is"):
        pj.binned_map_pol_nearest([(vals, vals, sky)], shape, wcs)
    with pytest.raises(ValueError, match="rcond_min"):
        pj.binned_map_pol_nearest([(vals, vals, sky, resp)], shape, wcs, rcond_min=0.0)


def test_header_and_bindings_declare_the_five_entries(pj):
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pixell_hip.h").read(), flags=re.S)
    julia = open(ROOT + "/julia/PixellHIP.jl").read()
    for name in ("pxl_sample_car_nearest_f64", "pxl_scatter_car_nearest_f64", "pxl_sample_car_pol_nearest_f64",
                 "pxl_scatter_car_pol_nearest_f64", "pxl_bin_car_pol_nearest_f64"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in pj._lib.SIGNATURES
        assert "ccall((:%s, libpixell_hip)" % name in julia, name
        assert hasattr(pj.load_library(), name)
    exports = " ".join(re.findall(r"^export (.*)$", julia, flags=re.M)).replace(",", " ").split()
    for fn in ("sample_nearest", "scatter_nearest!", "sample_pol_nearest", "scatter_pol_nearest!", "scatter_pol_weights_nearest!",
               "bin_pol_nearest!"):
        assert fn in exports, fn
    lib = pj.load_library()
    assert lib.pxl_bin_car_pol_nearest_f64(None, None, None, None, 0, None, None, None, None, None) == -22
    assert "WCS" in pj._lib.last_error()
