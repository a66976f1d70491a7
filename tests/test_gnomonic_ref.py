"""The long double Gnomonic yardstick (tests/gnomonic_ref.py) against mpmath at 50 digits evaluating the REFERENCE's own
formulas (tan_proj.jl:44-75: D = atan r, B = atan2(-X, Y), DEC = asin(..), RA = a0 + atan2(YY, XX)) from the same double inputs:
this checks the yardstick's algebra (the well-conditioned DEC = atan2(num, rho)) and its long double evaluation together, on
pixels on and next to a pole, rows beyond the pole (den < 0), points near the horizon and atan2's octant boundaries.
No GPU needed."""
import math

import numpy as np
import pytest

import gnomonic_ref as G

mpmath = pytest.importorskip("mpmath")
mp = mpmath.mp


def _need_longdouble():
    if np.finfo(np.longdouble).eps > 2e-19:
        pytest.skip("long double is not wider than double here")


def _wcs(cdelt_arcmin, crpix, crval):
    import pixell_jl_amd as pj
    return pj.Gnomonic((-cdelt_arcmin / 60, cdelt_arcmin / 60), crpix, crval)


def _mpl(v):
    """a long double as an mpf, exactly (its 64-bit significand is a double plus a double remainder)"""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))


def _mp_pix2sky(wcs, i, j):
    """tan_proj.jl:59-75 at 50 digits; X = (crpix - i) unit cdelt exactly (unit / scale, scale = 1 / cdelt)"""
    unit, cdelt = mp.mpf(wcs.unit), mp.mpf(wcs.cdelt[0])
    a0 = mp.mpf(G._reduced_crval0(wcs)) * mp.pi / 180
    d0 = mp.mpf(wcs.crval[1]) * mp.pi / 180
    X = (mp.mpf(wcs.crpix[0]) - mp.mpf(i)) * unit * cdelt
    Y = (mp.mpf(wcs.crpix[1]) - mp.mpf(j)) * unit * cdelt
    D = mp.atan(mp.sqrt(X * X + Y * Y))
    B = mp.atan2(-X, Y)
    XX = mp.sin(d0) * mp.sin(D) * mp.cos(B) + mp.cos(d0) * mp.cos(D)
    YY = mp.sin(D) * mp.sin(B)
    s = mp.sin(d0) * mp.cos(D) - mp.cos(d0) * mp.sin(D) * mp.cos(B)
    s = max(min(s, mp.mpf(1)), mp.mpf(-1))
    return a0 + mp.atan2(YY, XX), mp.asin(s)


def _mp_sky2pix(wcs, ra, dec):
    """tan_proj.jl:44-57 at 50 digits; also the plane radius r = tan c"""
    scale, unit = 1 / mp.mpf(wcs.cdelt[0]), mp.mpf(wcs.unit)
    a0 = mp.mpf(wcs.crval[0]) * mp.pi / 180
    d0 = mp.mpf(wcs.crval[1]) * mp.pi / 180
    d, da = mp.mpf(dec), mp.mpf(ra) - a0
    A = mp.cos(d) * mp.cos(da)
    cosc = mp.sin(d0) * mp.sin(d) + A * mp.cos(d0)
    F = scale / unit / cosc
    line = -F * (mp.cos(d0) * mp.sin(d) - A * mp.sin(d0))
    sample = -F * mp.cos(d) * mp.sin(da)
    return mp.mpf(wcs.crpix[0]) - sample, mp.mpf(wcs.crpix[1]) - line, mp.sqrt(1 - cosc * cosc) / cosc


def _points(wcs, rng, n):
    """pixel coordinates (doubles): the patch, the pole pixel and its neighbourhood, the plane's octant directions, and radii out
    to 89.9 degrees from the centre"""
    cx, cy = float(wcs.crpix[0]), float(wcs.crpix[1])
    pix = abs(wcs.cdelt[0]) * math.pi / 180
    ii = [cx + rng.uniform(-600, 600, n)]
    jj = [cy + rng.uniform(-600, 600, n)]
    px, py = G.pole_pixel(wcs)
    px, py = float(px), float(py)
    if abs(px) < 1e9 and abs(py) < 1e9:
        near = rng.uniform(-1.0, 1.0, (2, n // 4))
        ii += [np.array([px, np.nextafter(px, 0.0), px]), px + near[0], px + 3 * near[0]]
        jj += [np.array([py, py, np.nextafter(py, 1e300)]), py + near[1], py + 3 * near[1]]
    # octant boundaries of atan2 (directions k pi / 8 in the plane) and radii up to tan(89.9 deg) (the horizon)
    k = np.arange(n // 4)
    phi = (k % 16) * (math.pi / 8) + np.where(k % 3 == 0, 0.0, rng.uniform(-1e-9, 1e-9, k.size))
    rad = np.tan(np.radians(rng.uniform(0.0, 89.9, k.size))) / pix
    ii.append(cx + rad * np.cos(phi))
    jj.append(cy + rad * np.sin(phi))
    return np.concatenate(ii), np.concatenate(jj)


CASES = [(0.5, (512.5, 512.5), (40.0, 88.39)), (1.0, (384.5, 384.5), (-120.0, -89.2)), (0.5, (256.5, 256.5), (0.0, 90.0)),
         (0.5, (300.0, 200.5), (200.0, -90.0)), (1.0, (1000.5, 900.5), (10.0, 60.0)), (1.0, (1000.5, 900.5), (-720.5, -30.0)),
         (0.5, (913.5, 912.5), (97.5, -7.5)), (0.5, (4096.5, 4096.5), (40.0, -25.0)), (1.0, (512.5, 512.5), (33.0, 45.0))]


@pytest.mark.parametrize("cdelt,crpix,crval", CASES)
def test_yardstick_matches_mpmath(cdelt, crpix, crval):
    _need_longdouble()
    mp.dps = 50
    wcs = _wcs(cdelt, crpix, crval)
    rng = np.random.default_rng(int(abs(crval[1]) * 100) + 7)
    ii, jj = _points(wcs, rng, 400)
    ra, dec = G.tan_pix2sky(wcs, ii, jj)
    X, Y = G.plane(wcs, ii, jj)
    t = G.TanParams(wcs)
    den = (t.sd0 * Y + t.cd0).astype(float)
    cover = {"beyond pole (den < 0)": (den < 0).sum(), "near horizon (r > 10)": (G.plane_radius(wcs, ii, jj) > 10).sum()}
    e_ra = e_dec = 0.0
    for k in range(ii.size):
        mra, mdec = _mp_pix2sky(wcs, float(ii[k]), float(jj[k]))
        e_dec = max(e_dec, abs(float(_mpl(dec[k]) - mdec)))
        d = float(_mpl(ra[k]) - mra)
        d = abs((d + math.pi) % (2 * math.pi) - math.pi)
        e_ra = max(e_ra, d * math.cos(float(mdec)))
    assert e_dec <= 1e-18 and e_ra <= 1e-18, (e_ra, e_dec)
    assert cover["near horizon (r > 10)"] > 0, cover
    # sky2pix at the (rounded) sky positions of the same points, those in front of the tangent plane
    rad, decd = ra.astype(float), dec.astype(float)
    x, y, cosc = G.tan_sky2pix(wcs, rad, decd)
    su = abs(float(t.su))
    worst = 0.0
    for k in range(ii.size):
        if not float(cosc[k]) > 1e-6:
            continue
        mx, my, r = _mp_sky2pix(wcs, float(rad[k]), float(decd[k]))
        bar = 1e-18 * su * (1 + float(r) ** 2)
        worst = max(worst, abs(float(_mpl(x[k]) - mx)) / bar, abs(float(_mpl(y[k]) - my)) / bar)
    assert worst <= 1.0, worst
    print("%s: long double vs mpmath  ra*cos(dec) %.2g  dec %.2g rad  sky2pix %.2g of 1e-18 scale (1 + r^2); %s"
          % (crval, e_ra, e_dec, worst, cover))


def test_yardstick_covers_pole_rows_and_octants():
    """the sample sets above reach what they are meant to: a pixel within 1e-12 of a pole, rows beyond it, DEC on both sides of
    +-45 degrees (the octant boundary of atan2(num, rho)), and RA - a0 in all four quadrants"""
    _need_longdouble()
    wcs = _wcs(0.5, (512.5, 512.5), (40.0, 88.39))
    ii, jj = _points(wcs, np.random.default_rng(1), 400)
    ra, dec = G.tan_pix2sky(wcs, ii, jj)
    X, Y = G.plane(wcs, ii, jj)
    t = G.TanParams(wcs)
    den = (t.sd0 * Y + t.cd0).astype(float)
    assert (np.abs(dec.astype(float) - math.pi / 2) < 1e-12).any()
    assert (den < 0).sum() > 10 and (den > 0).sum() > 10
    assert (dec.astype(float) > math.pi / 4).any() and (dec.astype(float) < math.pi / 4).any()
    q = np.floor((ra - t.a0).astype(float) / (math.pi / 2)) % 4
    assert set(q.astype(int)) == {0, 1, 2, 3}


def test_conditioning_term_is_the_first_order_change():
    """the input terms against a direct first-order estimate: at a generic point, d0's move shifts DEC by about its own size, and
    on the pole pixel RA is undefined (a term of order pi: no RA bound is implied there)"""
    _need_longdouble()
    wcs = _wcs(0.5, (512.5, 512.5), (40.0, 60.0))
    tra, tdec = G.tan_pix2sky_cond(wcs, np.array([512.5]), np.array([512.5]))
    d0 = math.radians(60.0)
    # at the tangent point DEC = d0 exactly: the d0 move (3 U d0) plus sin d0's and cos d0's (2 U each, weighted by cos / sin)
    want = G.U * (3 * d0 + 2 * math.sin(d0) * math.cos(d0) + 2 * math.cos(d0) * math.sin(d0))
    assert abs(tdec[0] - want) <= 1e-3 * want, (tdec[0], want)
    px, py = G.pole_pixel(wcs)
    tra, tdec = G.tan_pix2sky_cond(wcs, np.array([float(px)]), np.array([float(py)]))
    assert tdec[0] < 1e-15 and tra[0] > 0.1
