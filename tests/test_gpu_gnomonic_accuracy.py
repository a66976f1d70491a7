"""The Gnomonic (TAN) evaluators on the device, every point held to a bound of its own against the well-conditioned long double
yardstick of tests/gnomonic_ref.py (not an L1 sum, not the oracle's error):

  DEC      |dDEC| <= 2 ulp(DEC) + 1.2e-16 + T_dec
           pxl_fm_asin / asin_w <= 0.8 ulp and the final rounding (tests/test_fastmath.py): 2 ulp of the angle with room; the
           sine's numerator num = sin d0 - cos d0 Y rounds twice, <= 2 U max(|sin d0|, |cos d0 Y|) <= 2 U s absolute, and
           DEC = atan2(num, rho) moves by rho / s^2 <= 1 / s per unit of num: <= 2 U = 1.1e-16 -> 1.2e-16.  No 1 / cos(DEC).
  RA       |dRA| <= 2 ulp(RA - a0) + ulp(RA) + 2.5e-16 / cos(DEC) + T_ra
           pxl_fm_atan2 <= 1.6 ulp (test_fastmath.py) -> 2 ulp of RA - a0; the final a0 + rounds once (ulp(RA) with a0's own
           rounding in T_ra); den = sin d0 Y + cos d0 rounds twice, <= 2 U s absolute, and atan2(-X, den) moves by
           |X| / rho^2 <= 1 / rho = 1 / (s cos DEC) per unit of den: 2 U / cos DEC = 2.2e-16 / cos DEC -> 2.5e-16 / cos DEC.
           (|dRA| cos DEC <= 2.5e-16 + ...: RA is a longitude, undefined on the pole itself.)
  sky2pix  |dx|, |dy| <= C U (scale / unit)(1 + r^2) + ulp(x) / 2 + T_x,  C = 5 sqrt(2) + 1 = 8.1
           cos c and the two numerators are sums of products of pxl_fm_sincos values (<= 1.5 ulp of 1 each) with sin d0, cos d0:
           <= 5 U absolute each; through F = (scale / unit) / cos c, with r = tan c, the offset moves by
           su 5 U (1 + r) sqrt(1 + r^2) <= 5 sqrt(2) U su (1 + r^2), and F's quotient and product round: + 2 U su r <= U su (1 + r^2).
           The final crpix - SAMPLE rounds once: ulp(x) / 2.
T_* are the per-point input-conditioning terms of gnomonic_ref.py (the device's rounded X, Y, a0, d0, sin d0, cos d0, scale / unit,
ra - a0 each moved by its own rounding).  Every case prints its worst error as a fraction of its bound."""
import math

import numpy as np
import pytest

import gnomonic_ref as G
from conftest import bits_equal
from gnomonic_ref import DEC_ABS, U, pix2sky_bounds

torch = pytest.importorskip("torch")
from gpu_support import device, to_dev
pytestmark = pytest.mark.gpu

C_S2P = 5 * math.sqrt(2) + 1
PXL_TILED_TOL = 1e-10             # pxl_sample.h: the tiled interpolant's per-tile check, in source pixels


@pytest.fixture(scope="module")
def dev():
    d = device()
    if np.finfo(np.longdouble).eps > 2e-19:
        pytest.skip("long double is not wider than double here")
    return d


_ulp = G.ulp


def check_pix2sky(tag, wcs, ii, jj, ra, dec, grid=False):
    """device (ra, dec) at pixel coordinates (ii, jj) against the yardstick; returns the worst fraction of the bound"""
    ra, dec = np.asarray(ra, dtype=np.float64).ravel(), np.asarray(dec, dtype=np.float64).ravel()
    ii, jj = np.asarray(ii, dtype=np.float64).ravel(), np.asarray(jj, dtype=np.float64).ravel()
    tra, tdec, b_ra, b_dec = pix2sky_bounds(wcs, ii, jj, grid)
    assert np.isfinite(ra).all() and np.isfinite(dec).all(), tag
    e_dec = np.abs((dec - tdec).astype(np.float64))
    e_ra = G.fold_ra(ra - tra)
    q_dec, q_ra = e_dec / b_dec, e_ra / b_ra
    k, m = int(np.argmax(q_dec)), int(np.argmax(q_ra))
    print("%-44s n=%-8d DEC worst %.3f of its bound (%.2e rad at dec %.6f)   RA worst %.3f (%.2e rad)"
          % (tag, ii.size, q_dec[k], e_dec[k], float(tdec[k]), q_ra[m], e_ra[m]))
    assert q_dec[k] <= 1.0, (tag, "DEC", float(ii[k]), float(jj[k]), float(dec[k]), float(tdec[k]), float(e_dec[k]), float(b_dec[k]))
    assert q_ra[m] <= 1.0, (tag, "RA", float(ii[m]), float(jj[m]), float(ra[m]), float(tra[m]), float(e_ra[m]), float(b_ra[m]))
    return max(q_dec[k], q_ra[m])


def check_sky2pix(tag, wcs, ra, dec, x, y):
    """device (x, y) at sky positions (ra, dec) against the yardstick, for the points in front of the tangent plane"""
    tx, ty, cosc = G.tan_sky2pix(wcs, ra, dec)
    cx, cy = G.tan_sky2pix_cond(wcs, ra, dec)
    ok = (cosc > 0.05).astype(bool)
    c64 = cosc.astype(np.float64)
    r2 = np.where(ok, (1 - c64 * c64) / np.maximum(c64 * c64, 1e-300), 0.0)
    su = abs(float(G.TanParams(wcs).su))
    worst = 0.0
    for name, got, ref, cond in (("x", x, tx, cx), ("y", y, ty, cy)):
        got = np.asarray(got, dtype=np.float64)
        assert np.isfinite(got[ok]).all(), tag
        err = np.abs((got - ref).astype(np.float64))
        bound = C_S2P * U * su * (1 + r2) + _ulp(ref.astype(np.float64)) / 2 + cond
        q = np.where(ok, err / bound, 0.0)
        k = int(np.argmax(q))
        assert q[k] <= 1.0, (tag, name, float(ra[k]), float(dec[k]), float(got[k]), float(ref[k]), float(err[k]), float(bound[k]))
        worst = max(worst, float(q[k]))
    print("%-44s n=%-8d sky2pix worst %.3f of its bound" % (tag, int(ok.sum()), worst))
    return worst


def run_pix2sky_both_paths(pj, dev, shape, wcs, ii, jj):
    """pxl_pix2sky_tan_f64 on 16-byte aligned arrays (k_tan_points<true>) and on views offset by one element (the scalar path):
    the same evaluator per element, so the same bits"""
    ra, dec = pj.pix2sky((shape, wcs), to_dev(ii, dev), to_dev(jj, dev))
    bi = torch.empty(ii.size + 1, dtype=torch.float64, device=dev)
    bj = torch.empty(ii.size + 1, dtype=torch.float64, device=dev)
    bi[1:].copy_(to_dev(ii, dev))
    bj[1:].copy_(to_dev(jj, dev))
    assert bi[1:].data_ptr() % 16 == 8
    ra2, dec2 = pj.pix2sky((shape, wcs), bi[1:], bj[1:])
    ra, dec, ra2, dec2 = (t.cpu().numpy() for t in (ra, dec, ra2, dec2))
    assert bits_equal(ra, ra2) and bits_equal(dec, dec2)
    return ra, dec


def run_sky2pix_both_paths(pj, dev, shape, wcs, ra, dec):
    x, y = pj.sky2pix((shape, wcs), to_dev(ra, dev), to_dev(dec, dev))
    br = torch.empty(ra.size + 1, dtype=torch.float64, device=dev)
    bd = torch.empty(ra.size + 1, dtype=torch.float64, device=dev)
    br[1:].copy_(to_dev(ra, dev))
    bd[1:].copy_(to_dev(dec, dev))
    x2, y2 = pj.sky2pix((shape, wcs), br[1:], bd[1:])
    x, y, x2, y2 = (t.cpu().numpy() for t in (x, y, x2, y2))
    assert bits_equal(x, x2) and bits_equal(y, y2)
    return x, y


def _scatter(wcs, rng, n, max_deg=85.0):
    """pixel coordinates out to max_deg from the tangent point, the plane's octant directions first"""
    pix = abs(wcs.cdelt[0]) * math.pi / 180
    rad = np.tan(np.radians(rng.uniform(0.0, max_deg, n))) / pix
    phi = rng.uniform(0.0, 2 * np.pi, n)
    phi[:64] = np.arange(64) * (np.pi / 32)
    return float(wcs.crpix[0]) + rad * np.cos(phi), float(wcs.crpix[1]) + rad * np.sin(phi)


def _near_pole(wcs, rng, n, radius=3.0):
    px, py = (float(v) for v in G.pole_pixel(wcs))
    ii = np.concatenate([[px, np.nextafter(px, 0.0)], px + rng.uniform(-radius, radius, n)])
    jj = np.concatenate([[py, py], py + rng.uniform(-radius, radius, n)])
    return ii, jj


def _posmap_rows(pj, dev, shape, wcs, row0=0, nrows=None):
    nrows = shape[1] - row0 if nrows is None else nrows
    ra, dec = pj.posmap(shape, wcs, device=dev, row0=row0, nrows=nrows)
    jj, ii = np.meshgrid(np.arange(row0 + 1, row0 + nrows + 1, dtype=float), np.arange(1, shape[0] + 1, dtype=float), indexing="ij")
    return ii, jj, ra.data.cpu().numpy(), dec.data.cpu().numpy()


def _grid_taken(wcs, shape, nrows):
    """pxl_posmap_tan_f64's choice of k_posmap_tan_grid (host arithmetic)"""
    uos = wcs.unit * wcs.cdelt[0]
    return abs(uos) * 128 <= 0.04 and abs(math.cos(wcs.crval[1] * math.pi / 180)) >= 0.3 and shape[0] >= 128 and nrows >= 8


# ---- pix2sky / sky2pix on scattered points -----------------------------------------------------------

POLAR = [(d, res) for d in (60.0, 80.0, 88.39, 89.2, 89.9, 90.0, -60.0, -80.0, -88.39, -89.2, -89.9, -90.0) for res in (0.5,)]


@pytest.mark.parametrize("d0,res", POLAR)
def test_points_polar_centres(pj, dev, d0, res):
    """Patches centred at |dec| 60 ... 90 in both hemispheres: points out to 85 degrees from the centre (rows beyond the pole,
    every octant of atan2), dense sampling within 3 pixels of the pole (the pole pixel itself first), both entry paths; then
    sky2pix at the yardstick's positions of the same points."""
    rng = np.random.default_rng(int(abs(d0) * 1000) + (d0 < 0))
    wcs = pj.Gnomonic((-res / 60, res / 60), (512.5, 512.5), (float(rng.uniform(-180, 180)), d0))
    shape = (1024, 1024)
    i1, j1 = _scatter(wcs, rng, 40001)
    i2, j2 = _near_pole(wcs, rng, 20000)
    i3, j3 = 512.5 + rng.uniform(-512, 512, 40000), 512.5 + rng.uniform(-512, 512, 40000)
    ii, jj = np.concatenate([i1, i2, i3]), np.concatenate([j1, j2, j3])
    ra, dec = run_pix2sky_both_paths(pj, dev, shape, wcs, ii, jj)
    check_pix2sky("pix2sky centre %+.2f" % d0, wcs, ii, jj, ra, dec)
    check_pix2sky("pix2sky centre %+.2f, within 3 px of the pole" % d0, wcs, i2, j2, ra[i1.size:i1.size + i2.size],
                  dec[i1.size:i1.size + i2.size])
    tra, tdec = G.tan_pix2sky(wcs, ii, jj)
    sra, sdec = tra.astype(np.float64), tdec.astype(np.float64)
    x, y = run_sky2pix_both_paths(pj, dev, shape, wcs, sra, sdec)
    check_sky2pix("sky2pix centre %+.2f" % d0, wcs, sra, sdec, x, y)


@pytest.mark.parametrize("crval", [(97.5, -7.5), (0.0, 0.0), (-170.0, 45.0), (-720.5, -30.0), (359.0, 30.0)])
def test_points_wide_fields(pj, dev, crval):
    """Points out to 85 degrees from centres across the sky, an RA of many turns (-720.5) among them."""
    rng = np.random.default_rng(int(crval[0] * 10 + crval[1]) & 0xffff)
    wcs = pj.Gnomonic((-1.0 / 60, 1.0 / 60), (1000.5, 900.5), crval)
    shape = (2000, 1800)
    ii, jj = _scatter(wcs, rng, 200001)
    ra, dec = run_pix2sky_both_paths(pj, dev, shape, wcs, ii, jj)
    check_pix2sky("pix2sky wide %s" % (crval,), wcs, ii, jj, ra, dec)
    tra, tdec = G.tan_pix2sky(wcs, ii, jj)
    sra = tra.astype(np.float64) + (float(crval[0]) - G._reduced_crval0(wcs)) * math.pi / 180    # the device's turn
    sdec = tdec.astype(np.float64)
    x, y = run_sky2pix_both_paths(pj, dev, shape, wcs, sra, sdec)
    check_sky2pix("sky2pix wide %s" % (crval,), wcs, sra, sdec, x, y)


def test_points_reference_and_bench_patches(pj, dev, literals):
    """The reference's 1827 x 1825 patch (tests/golden/reference_literals.json) and bench.py's 8192^2 patch of 0.5' at (40, -25),
    sampled, through both entry paths and sky2pix."""
    g = literals["gnomonic"]
    rng = np.random.default_rng(5)
    for tag, shape, wcs in (("reference patch", tuple(g["shape"]), pj.Gnomonic(g["cdelt"], g["crpix"], g["crval"])),
                            ("bench patch", (8192, 8192), pj.Gnomonic((-0.5 / 60, 0.5 / 60), (4096.5, 4096.5), (40.0, -25.0)))):
        ii, jj = rng.uniform(1, shape[0], 200001), rng.uniform(1, shape[1], 200001)
        ra, dec = run_pix2sky_both_paths(pj, dev, shape, wcs, ii, jj)
        check_pix2sky("pix2sky " + tag, wcs, ii, jj, ra, dec)
        x, y = run_sky2pix_both_paths(pj, dev, shape, wcs, ra, dec)
        check_sky2pix("sky2pix " + tag, wcs, ra, dec, x, y)


def test_points_wave_votes(pj, dev):
    """k_tan_points takes each wave (64 lanes = 128 consecutive points) through a vote: asin<1> when every sine is within 1/2,
    else the two-half asin_w; atan2<TAME> when every lane has den > 0, else the general atan2.  Batches of 128 points are built
    to be all-small, all-big, mixed, all beyond the pole (den < 0) and mixed in den, so that every specialisation runs."""
    rng = np.random.default_rng(99)
    wcs = pj.Gnomonic((-1.0 / 60, 1.0 / 60), (1000.5, 900.5), (25.0, 35.0))
    shape = (2000, 1800)
    ii, jj = _scatter(wcs, rng, 400000, max_deg=80.0)
    _, tdec = G.tan_pix2sky(wcs, ii, jj)
    X, Y = G.plane(wcs, ii, jj)
    t = G.TanParams(wcs)
    den = (t.sd0 * Y + t.cd0).astype(np.float64)
    sdec = np.abs(np.sin(tdec.astype(np.float64)))
    pools = {"small": (sdec < 0.49) & (den > 0), "big": (sdec > 0.51) & (den > 0), "beyond": (sdec > 0.51) & (den < 0)}
    idx = {k: np.flatnonzero(v) for k, v in pools.items()}
    assert all(v.size >= 128 * 40 for v in idx.values()), {k: v.size for k, v in idx.items()}
    groups = []
    for g in range(40):
        sl = slice(128 * g, 128 * (g + 1))
        half = slice(64 * g, 64 * (g + 1))
        groups += [idx["small"][sl], idx["big"][sl], idx["beyond"][sl],
                   np.concatenate([idx["small"][half], idx["big"][half]]),          # mixed halves, den > 0
                   np.concatenate([idx["big"][half], idx["beyond"][half]]),         # big sines, den of both signs
                   np.concatenate([idx["small"][half][:1], idx["big"][sl][1:]])]    # one small lane among big ones
    order = np.concatenate(groups)
    assert order.size % 128 == 0
    ip, jp = ii[order], jj[order]
    ra, dec = run_pix2sky_both_paths(pj, dev, shape, wcs, ip, jp)
    check_pix2sky("pix2sky wave votes", wcs, ip, jp, ra, dec)


# ---- posmap: k_posmap_tan and k_posmap_tan_grid ------------------------------------------------------

@pytest.mark.parametrize("d0", [88.39, -88.39, 89.2, 90.0, -90.0, 80.0, 60.0, -60.0])
def test_posmap_polar(pj, dev, d0):
    """The posmap of 512^2 patches of 0.5' (the pole inside for |d0| >= 88.3; rows beyond it, den <= 0, in whole waves and in
    mixed ones): the full map and row windows (row0 / nrows) that are bit-identical to its rows.  |d0| >= 72.5: k_posmap_tan
    (its waves vote asin<1> / asin_w<2> / asin_w<0>); 60: k_posmap_tan_grid."""
    n = 512
    wcs = pj.Gnomonic((-0.5 / 60, 0.5 / 60), (n / 2 + 0.5, n / 2 + 0.5), (40.0, d0))
    ii, jj, ra, dec = _posmap_rows(pj, dev, (n, n), wcs)
    grid = _grid_taken(wcs, (n, n), n)
    assert grid == (abs(d0) < 72.5)
    check_pix2sky("posmap %s %+.2f" % ("grid" if grid else "per-pixel", d0), wcs, ii, jj, ra, dec, grid=grid)
    for r0, nr in ((0, 8), (100, 64), (255, 3), (n - 65, 65)):
        _, _, wr, wd = _posmap_rows(pj, dev, (n, n), wcs, r0, nr)
        if _grid_taken(wcs, (n, n), nr) == grid:
            assert bits_equal(wr, ra[r0:r0 + nr]) and bits_equal(wd, dec[r0:r0 + nr]), (d0, r0, nr)
        else:
            check_pix2sky("posmap window %+.2f rows %d+%d" % (d0, r0, nr), wcs, ii[r0:r0 + nr], jj[r0:r0 + nr], wr, wd)


def test_posmap_pole_on_a_pixel_centre(pj, dev):
    """The pole exactly on a pixel centre (crpix moved by the fraction), as test_gnomonic_celestial_pole_is_finite_on_device
    places it: the pole pixel's DEC is +-pi/2 to the per-point bound, every pixel held to its own."""
    for d0, res in ((88.0, 1.0), (-89.5, 0.5), (75.0, 4.0)):
        wcs0 = pj.Gnomonic((-res / 60, res / 60), (256.5, 256.5), (33.0, d0))
        px, py = (float(v) for v in G.pole_pixel(wcs0))
        wcs = pj.Gnomonic(wcs0.cdelt, (256.5 + (round(px) - px), 256.5 + (round(py) - py)), (33.0, d0))
        ip, jp = int(round(px)), int(round(py))
        shape = (max(512, ip + 8), max(512, jp + 8))
        ii, jj, ra, dec = _posmap_rows(pj, dev, shape, wcs)
        check_pix2sky("posmap pole on pixel (%d, %d), %+.1f" % (ip, jp, d0), wcs, ii, jj, ra, dec)
        pole = math.copysign(math.pi / 2, d0)
        assert abs(dec[jp - 1, ip - 1] - pole) <= 2 * np.spacing(abs(pole)) + DEC_ABS, (d0, dec[jp - 1, ip - 1])


def test_posmap_grid_bench_and_reference(pj, dev, literals):
    """k_posmap_tan_grid on the bench patch (8192^2 of 0.5' at (40, -25)) in row windows of 64 at the top, middle and bottom, and
    the reference's whole 1827 x 1825 patch (every 3rd row checked)."""
    n = 8192
    wcs = pj.Gnomonic((-0.5 / 60, 0.5 / 60), (n / 2 + 0.5, n / 2 + 0.5), (40.0, -25.0))
    for r0 in (0, 4064, n - 64):
        assert _grid_taken(wcs, (n, n), 64)
        ii, jj, ra, dec = _posmap_rows(pj, dev, (n, n), wcs, r0, 64)
        check_pix2sky("posmap grid bench rows %d+64" % r0, wcs, ii, jj, ra, dec, grid=True)
    g = literals["gnomonic"]
    shape = tuple(g["shape"])
    wcs = pj.Gnomonic(g["cdelt"], g["crpix"], g["crval"])
    assert _grid_taken(wcs, shape, shape[1])
    ii, jj, ra, dec = _posmap_rows(pj, dev, shape, wcs)
    check_pix2sky("posmap grid reference patch", wcs, ii[::3], jj[::3], ra[::3], dec[::3], grid=True)


# ---- CAR -> TAN reprojection of a polar patch ----------------------------------------------------------

def test_reproject_car_to_tan_polar_patch(pj, dev, monkeypatch):
    """A 0.5' TAN patch centred at dec 88.39 (the pole and the rows beyond it inside) reprojected from the top 701 rows of the
    0.5' full-sky CAR map with a ramp source (plane 0 = column index, plane 1 = row index: bilinear interpolation reproduces an
    affine field, so in every interior cell the output planes ARE the source coordinates the kernel used), through the one-shot
    entry, a plan and the per-pixel path.  Source coordinates against the yardstick's: x moves by dRA / pixel, y by dDEC /
    pixel, with the pix2sky bounds above, 8 ulp of the coordinate for the CAR sky2pix, and PXL_TILED_TOL on the tiled paths."""
    from test_gpu_interpolated import _car_sky2pix_ld, _ramp, _run_generic
    fshape, fwcs = pj.fullsky_geometry(2 * math.pi / 43200)
    sshape, swcs = pj.slice_geometry(fshape, fwcs, None, (fshape[1] - 700, fshape[1]))
    sshape = (sshape[0], sshape[1])
    oshape = (512, 512)
    owcs = pj.Gnomonic((-0.5 / 60, 0.5 / 60), (256.5, 256.5), (40.0, 88.39))
    src = _ramp(sshape, dev)
    nxo, nyo = oshape
    jj, ii = np.meshgrid(np.arange(1, nyo + 1, dtype=float), np.arange(1, nxo + 1, dtype=float), indexing="ij")
    tra, tdec, b_ra, b_dec = pix2sky_bounds(owcs, ii.ravel(), jj.ravel())
    x, y = _car_sky2pix_ld(swcs, sshape, tra, tdec)
    pix = abs(swcs.cdelt[0] * swcs.unit)
    interior = (x >= 1 + 1e-6) & (x < sshape[0] - 1e-6) & (y >= 1 + 1e-6) & (y < sshape[1] - 1e-6)
    # away from the RA seam of the periodic source (the ramp is not affine across it) -- and off the pole itself, where a pixel
    # of RA is an arbitrarily small distance
    xx = x.astype(np.float64)
    interior &= (xx > 2) & (xx < sshape[0] - 2) & (np.cos(tdec.astype(np.float64)) > 1e-6)
    assert interior.mean() > 0.9, interior.mean()
    try:
        for how in ("tiled", "plan", "exact"):
            got, _ = _run_generic(pj, dev, src, swcs, oshape, owcs, how, monkeypatch)
            got = got.cpu().numpy().reshape(2, -1)
            worst = 0.0
            for plane, ref, bang in ((0, x, b_ra), (1, y, b_dec)):
                r64 = ref.astype(np.float64)
                mag = np.maximum(np.abs(r64), np.abs(r64 - swcs.crpix[plane]))
                bound = 8 * np.spacing(mag) + bang / pix + (0.0 if how == "exact" else PXL_TILED_TOL)
                err = np.abs((got[plane] - ref).astype(np.float64))
                q = np.where(interior, err / bound, 0.0)
                k = int(np.argmax(q))
                assert q[k] <= 1.0, (how, plane, float(err[k]), float(bound[k]), float(tdec[k]))
                worst = max(worst, float(q[k]))
            print("CAR->TAN polar patch (%s): worst %.3f of the bound over %d interior pixels" % (how, worst, int(interior.sum())))
    finally:
        del src
        torch.cuda.empty_cache()
