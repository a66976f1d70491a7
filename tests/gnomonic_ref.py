"""Extended-precision yardstick for the Gnomonic (TAN) evaluators, tan_proj.jl:44-75, in numpy long double (x87: 64-bit
significand here).  A helper module of the tests, not a test module.

pix2sky is evaluated in a form that is well conditioned everywhere, the poles included.  With the plane coordinates
X = (crpix_x - i) unit / scale, Y = (crpix_y - j) unit / scale and
    den = sin d0 Y + cos d0,   num = sin d0 - cos d0 Y,   rho = sqrt(X^2 + den^2)     (num^2 + rho^2 = 1 + X^2 + Y^2)
the sky position is
    RA  = a0 + atan2(-X, den),   DEC = atan2(num, rho).
(The reference's own sequence -- asin of a direction cosine -- loses 1 / cos(DEC) of its precision near a pole, in long double
as in double.)  sky2pix keeps the reference's operations (tan_proj.jl:44-57), which are well conditioned.

The *_cond functions give a per-point input-conditioning term: the change of the output when each rounded quantity the device
forms from its double inputs (the plane coordinates, a0, d0, sin d0, cos d0, scale / unit, ra - a0) is moved by its own rounding,
evaluated with this yardstick by central differences.  A device result can be off by that much without any error of its own
evaluation, so the per-point bounds of the accuracy tests add it; the moves are derived from the operations in pxl_tan.h
(tan_setup and the evaluators), not fitted.
"""
import math

import numpy as np

L = np.longdouble
PI_L = L("3.14159265358979323846264338327950288")
U = 2.0 ** -53                     # unit roundoff of a double

# Relative moves of the device's rounded quantities (pxl_tan.h), in units of U:
H_PLANE = 4      # X = fl(fl(crpix - i) * uos), uos = fl(unit / fl(1 / cdelt)): four roundings (likewise Y)
H_ANGLE = 3      # a0 = fl(crval * fl(fl(pi) / 180)): three roundings (likewise d0)
H_TRIG = 2       # sin d0, cos d0 from the library: below one ulp, i.e. 2 U relative
H_SU = 2         # su = fl(fl(1 / cdelt) / unit): two roundings
H_DA = 1         # ra - a0: one rounding (a0's own moves are the a0 term)


# the device's own evaluation error in the pix2sky bounds (tests/test_gpu_gnomonic_accuracy.py derives them)
DEC_ABS = 1.2e-16                 # DEC: the two roundings of num = sin d0 - cos d0 Y, through d DEC / d num <= 1 / s
RA_ABS = 2.5e-16                  # RA * cos DEC: the two roundings of den = sin d0 Y + cos d0, through |X| / rho^2
GRID_EXTRA = 2.0 ** -54           # k_posmap_tan_grid: its node check tolerance 2^-55 and the interpolant's rounding


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(L)


def _reduced_crval0(wcs):
    """crval[0] folded into [-180, 180) (math.fmod and the subtraction are exact): the yardstick's a0 keeps long double precision
    for an RA of many turns; its RA then differs from the device's by whole turns (compare with fold_ra)."""
    c = math.fmod(float(wcs.crval[0]), 360.0)
    return c - 360.0 if c >= 180.0 else (c + 360.0 if c < -180.0 else c)


class TanParams:
    """The long double constants of a Gnomonic WCS (a0, d0 = crval pi / 180; scale = 1 / cdelt)."""

    def __init__(self, wcs):
        self.unit = L(wcs.unit)
        self.cdelt = L(wcs.cdelt[0])
        self.scale = L(1) / self.cdelt
        self.uos = self.unit * self.cdelt              # unit / scale
        self.su = self.scale / self.unit
        self.a0 = L(_reduced_crval0(wcs)) * (PI_L / 180)
        self.d0 = L(wcs.crval[1]) * (PI_L / 180)
        self.sd0, self.cd0 = np.sin(self.d0), np.cos(self.d0)
        self.cpx, self.cpy = L(wcs.crpix[0]), L(wcs.crpix[1])
        # magnitudes of the device's own constants (a0 unreduced: an RA of many turns rounds like its size)
        self.a0_dev = abs(float(wcs.crval[0]) * math.pi / 180)


def plane(wcs, ii, jj):
    """X, Y (long double) of pixel coordinates ii, jj (1-based, doubles)"""
    t = TanParams(wcs)
    return (t.cpx - _ld(ii)) * t.uos, (t.cpy - _ld(jj)) * t.uos


def _p2s(X, Y, a0, sd0, cd0):
    den = sd0 * Y + cd0
    num = sd0 - cd0 * Y
    return a0 + np.arctan2(-X, den), np.arctan2(num, np.sqrt(X * X + den * den))


def tan_pix2sky(wcs, ii, jj):
    """(RA, DEC) in long double; RA = a0 + atan2(..) with a0 folded to [-pi, pi)"""
    t = TanParams(wcs)
    X, Y = plane(wcs, ii, jj)
    return _p2s(X, Y, t.a0, t.sd0, t.cd0)


def fold_ra(d):
    """|a difference of two RA values| folded across whole turns (atan2's cut, RA of many turns), as float64"""
    d = np.asarray(d, dtype=L)
    return np.abs(((d + PI_L) % (2 * PI_L)) - PI_L).astype(np.float64)


def _central(f, base, k, h, fold_first=False):
    """|f(.., x_k + h, ..) - f(.., x_k - h, ..)| / 2 for each output of f (the first folded across whole turns: an RA)"""
    lo, hi = list(base), list(base)
    lo[k] = base[k] - h
    hi[k] = base[k] + h
    out = []
    for n, (a, b) in enumerate(zip(f(*lo), f(*hi))):
        out.append((fold_ra(b - a) if fold_first and n == 0 else np.abs((b - a).astype(np.float64))) / 2)
    return out


def tan_pix2sky_cond(wcs, ii, jj):
    """Per-point input-conditioning terms (term_ra, term_dec), float64 radians: X, Y, a0, d0, sin d0, cos d0 each moved by its
    own rounding (H_* above), the changes of RA and DEC summed in magnitude."""
    t = TanParams(wcs)
    X, Y = plane(wcs, ii, jj)

    def f(X, Y, a0, d0, sd0, cd0):
        # d0 moves sin d0 and cos d0 together; sd0 / cd0 move on their own (the library's roundings)
        return _p2s(X, Y, a0, sd0 + (np.sin(d0) - t.sd0), cd0 + (np.cos(d0) - t.cd0))

    base = [X, Y, t.a0, t.d0, t.sd0, t.cd0]
    moves = [H_PLANE * U * np.abs(X), H_PLANE * U * np.abs(Y), L(H_ANGLE * U * t.a0_dev), H_ANGLE * U * abs(t.d0),
             H_TRIG * U * abs(t.sd0), H_TRIG * U * abs(t.cd0)]
    tra = np.zeros(np.shape(X))
    tdec = np.zeros(np.shape(X))
    for k, h in enumerate(moves):
        dr, dd = _central(f, base, k, L(h), fold_first=True)
        tra += dr
        tdec += dd
    return tra, tdec


def _s2p(da, sd, cd, sd0, cd0, su, cpx, cpy):
    """tan_proj.jl:44-57 (the reference's operations); also cos c, the cosine of the distance from the tangent point"""
    sa, ca = np.sin(da), np.cos(da)
    A = cd * ca
    cosc = sd0 * sd + A * cd0
    F = su / cosc
    line = -F * (cd0 * sd - A * sd0)
    sample = -F * cd * sa
    return cpx - sample, cpy - line, cosc


def tan_sky2pix(wcs, ra, dec):
    """(x, y, cos c) in long double for doubles ra, dec"""
    t = TanParams(wcs)
    dec = _ld(dec)
    da = _ld(ra) - L(float(wcs.crval[0])) * (PI_L / 180)
    return _s2p(da, np.sin(dec), np.cos(dec), t.sd0, t.cd0, t.su, t.cpx, t.cpy)


def tan_sky2pix_cond(wcs, ra, dec):
    """Per-point input-conditioning terms (term_x, term_y), float64 pixels: ra - a0 (a0's moves and the subtraction's rounding),
    d0, sin d0, cos d0 and scale / unit, each moved by its own rounding.  dec is the exact input: the sincos error bounds of
    pxl_fastmath.h are measured against the exact argument, reduction included."""
    t = TanParams(wcs)
    decl = _ld(dec)
    sd, cd = np.sin(decl), np.cos(decl)
    da = _ld(ra) - L(float(wcs.crval[0])) * (PI_L / 180)

    def f(da, d0, sd0, cd0, su):
        x, y, _ = _s2p(da, sd, cd, sd0 + (np.sin(d0) - t.sd0), cd0 + (np.cos(d0) - t.cd0), su, t.cpx, t.cpy)
        return x, y

    base = [da, t.d0, t.sd0, t.cd0, t.su]
    moves = [L(H_ANGLE * U * t.a0_dev) + H_DA * U * np.abs(da), H_ANGLE * U * abs(t.d0), H_TRIG * U * abs(t.sd0),
             H_TRIG * U * abs(t.cd0), H_SU * U * abs(t.su)]
    tx = np.zeros(np.shape(da))
    ty = np.zeros(np.shape(da))
    for k, h in enumerate(moves):
        dx, dy = _central(f, base, k, L(h))
        tx += dx
        ty += dy
    return tx, ty


def plane_radius(wcs, ii, jj):
    """r = tan(distance from the tangent point) of pixel coordinates, float64"""
    X, Y = plane(wcs, ii, jj)
    return np.sqrt((X * X + Y * Y).astype(np.float64))


def pole_pixel(wcs):
    """pixel coordinates (long double) of the celestial pole in front of the tangent plane (X = 0, den = 0: Y = -cot d0); the
    north pole for d0 > 0"""
    t = TanParams(wcs)
    Y = -t.cd0 / t.sd0
    return t.cpx, t.cpy - Y / t.uos


def pix2sky_bounds(wcs, ii, jj, grid=False):
    """yardstick (RA, DEC) in long double and the per-point bounds (b_ra, b_dec) on a device evaluation at (ii, jj):
    |dDEC| <= 2 ulp(DEC) + DEC_ABS + T_dec, |dRA| <= 2 ulp(RA - a0) + ulp(RA) + RA_ABS / cos DEC + T_ra (derived in
    tests/test_gpu_gnomonic_accuracy.py); grid: k_posmap_tan_grid's interpolated pixels, GRID_EXTRA and one ulp more"""
    tra, tdec = tan_pix2sky(wcs, ii, jj)
    cra, cdec = tan_pix2sky_cond(wcs, ii, jj)
    d64 = tdec.astype(np.float64)
    phi = (tra - TanParams(wcs).a0).astype(np.float64)
    with np.errstate(divide="ignore"):
        b_ra = 2 * ulp(phi) + ulp(tra.astype(np.float64) + (float(wcs.crval[0]) - _reduced_crval0(wcs)) * math.pi / 180) \
            + RA_ABS / np.cos(d64) + cra
    b_dec = 2 * ulp(d64) + DEC_ABS + cdec
    if grid:
        b_ra = b_ra + GRID_EXTRA + ulp(tra.astype(np.float64))
        b_dec = b_dec + GRID_EXTRA + ulp(d64)
    return tra, tdec, b_ra, b_dec
