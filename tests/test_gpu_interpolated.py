"""The two kernels that INTERPOLATE coordinates instead of evaluating them, held per pixel:

* k_posmap_tan_grid (pxl_tan.h): the Gnomonic posmap from one exact anchor per row and tile, closed-form differences at nine node
  columns and a degree-8 interpolant across the tile's 128 columns;
* k_reproject_generic_tiled3 (pxl_sample.h): the CAR <-> Gnomonic reprojection with the source coordinates interpolated per
  128 x 32 output tile (checked at twelve points per tile to PXL_TILED_TOL pixel).

Every bound below follows from the conditioning of the operation and the kernels' documented tolerances; none is fitted to a
measurement.  The extended-precision yardsticks are the reference's formulas (tan_proj.jl:44-75, car_proj.jl) in numpy long double.
Last: the one-shot generic entry must give the bits of a serial call while other one-shot calls run on other streams and threads."""
import math
import threading

import numpy as np
import pytest

import gnomonic_ref as G
from conftest import ARCMIN, DEG, bits_equal

torch = pytest.importorskip("torch")
from gpu_support import dev, to_dev
pytestmark = pytest.mark.gpu

L = np.longdouble
PI_L = L("3.14159265358979323846264338327950288")
PXL_TILED_TOL = 1e-10             # pxl_sample.h: the tiled interpolant's per-tile check, in source pixels
TG_W, TG_ROWS, TG_NODES, TG_SMAX = 128, 64, 9, 0.0625      # pxl_tan.h: the grid posmap's tile and small-angle limit


def _need_longdouble():
    if np.finfo(np.longdouble).eps > 2e-19:
        pytest.skip("long double is not wider than double here")


def _wrap(d):
    """a difference of two RA values, folded into [-pi, pi] (atan2's cut passes behind the pole)"""
    return np.abs((d + math.pi) % (2 * math.pi) - math.pi)


# ---- long-double yardsticks -----------------------------------------------------------------------

def _tan_pix2sky_ld(wcs, ii, jj):
    """the shared well-conditioned yardstick (tests/gnomonic_ref.py: DEC = atan2(num, rho), accurate on a pole as anywhere), with
    RA on the device's turn of a0"""
    ra, dec = G.tan_pix2sky(wcs, ii, jj)
    return ra + L(float(wcs.crval[0]) - G._reduced_crval0(wcs)) * (PI_L / 180), dec


def _tan_sky2pix_ld(wcs, ra, dec):
    """tan_proj.jl:44-57 in long double; also cos c, the cosine of the distance from the tangent point (visible: > 0)."""
    scale, unit = L(1.0) / L(wcs.cdelt[0]), L(wcs.unit)
    a0, d0 = L(wcs.crval[0]) * (PI_L / 180), L(wcs.crval[1]) * (PI_L / 180)
    sd, cd, sa, ca = np.sin(dec), np.cos(dec), np.sin(ra - a0), np.cos(ra - a0)
    A = cd * ca
    cosc = np.sin(d0) * sd + A * np.cos(d0)
    F = scale / unit / cosc
    line = -F * (np.cos(d0) * sd - A * np.sin(d0))
    sample = -F * cd * sa
    return L(wcs.crpix[0]) - sample, L(wcs.crpix[1]) - line, cosc


def _car_pix2sky_ld(wcs, ii, jj):
    u = L(wcs.unit)
    return (L(wcs.crval[0]) * u + (np.asarray(ii).astype(L) - L(wcs.crpix[0])) * (L(wcs.cdelt[0]) * u),
            L(wcs.crval[1]) * u + (np.asarray(jj).astype(L) - L(wcs.crpix[1])) * (L(wcs.cdelt[1]) * u))


def _ld_rewind(a, period, ref):
    half = period / 2
    return (ref + np.mod((a - ref) + half, period)) - half


def _car_sky2pix_ld(wcs, shape, ra, dec):
    """car_proj.jl:220-234 (the division form) with the safe rewind about the map centre (s2p_eval, oracle/pixell_oracle.c)."""
    u = L(wcs.unit)
    da, dd = L(wcs.cdelt[0]) * u, L(wcs.cdelt[1]) * u
    x = L(wcs.crpix[0]) + (ra - L(wcs.crval[0]) * u) / da
    y = L(wcs.crpix[1]) + (dec - L(wcs.crval[1]) * u) / dd
    x = _ld_rewind(x, abs(2 * PI_L / da), L(shape[0]) / 2 + 1)
    y = _ld_rewind(y, abs(2 * PI_L / dd), L(shape[1]) / 2 + 1)
    return x, y


# ---- A. k_posmap_tan_grid per pixel ---------------------------------------------------------------

def _grid_taken(wcs, shape, nrows):
    """pxl_posmap_tan_f64's choice of the grid kernel (host arithmetic)"""
    uos = wcs.unit * wcs.cdelt[0]
    return abs(uos) * TG_W <= 0.04 and abs(math.cos(wcs.crval[1] * math.pi / 180)) >= 0.3 and shape[0] >= TG_W and nrows >= 8


def _pp_bound(p, a0, is_ra, inf):
    """|grid - per-pixel| allowed at per-pixel values p: both evaluators' 1.5 ulp, one rounding and the 2^-55 node check
    (4 ulp + 2^-54), in ulp of what the last transcendental returns.  RA = a0 + atan2(..): the atan2 result is RA - a0, so its ulp
    is that of max(|RA|, |RA - a0|) (RA crosses zero on patches away from a0 = 0, where ulp(RA) alone means nothing).
    DEC: s = num * rsqrt(..) carries four roundings (the rsqrt's 1.5 ulp, num's two, the product) in each evaluator; in the small
    half of asin a relative error e of s is e |tan DEC| <= e / sqrt(3) of angle, 2 x 4 u |tan DEC| (u = 2^-53); the big half
    takes w = (1 - |s|) / 2 without cancellation (pxl_tan.h), which leaves each evaluator num's rounding, gnomonic_ref.DEC_ABS:
    the smaller of the two terms."""
    if is_ra:
        a = torch.maximum(p.abs(), (p - a0).abs())
        return 4 * (torch.nextafter(a, inf) - a) + 2.0 ** -54
    a = p.abs()
    return 4 * (torch.nextafter(a, inf) - a) + 2.0 ** -54 + torch.clamp(8 * 2.0 ** -53 * torch.tan(a), max=2 * G.DEC_ABS)


def _check_posmap(pj, O, dev, shape, wcs, block=1024, tag=""):
    """The posmap of (shape, wcs) against (1) the device's per-pixel evaluator (k_tan_points) on the same pixel centres,
    (2) the oracle over the whole map, (3) the long-double formula on every 61st row and on every tile-edge column of 200
    random rows.  Returns the maxima of |grid - (1)| / bound and of |grid - (2), (3)|."""
    nx, ny = shape
    a0 = wcs.crval[0] * math.pi / 180
    ra_m, dec_m = pj.posmap(shape, wcs, device=dev)
    ra_m, dec_m = ra_m.data, dec_m.data
    worst = {"pp": 0.0, "pp_abs": 0.0, "oracle": 0.0, "ld": 0.0}
    cols = torch.arange(1, nx + 1, dtype=torch.float64, device=dev)
    inf = torch.tensor(math.inf, dtype=torch.float64, device=dev)
    for r0 in range(0, ny, block):
        nr = min(block, ny - r0)
        jj = torch.arange(r0 + 1, r0 + nr + 1, dtype=torch.float64, device=dev)[:, None].expand(nr, nx).contiguous()
        ii = cols[None, :].expand(nr, nx).contiguous()
        pra, pdec = pj.pix2sky((shape, wcs), ii, jj, safe=False)
        gra, gdec = ra_m[r0:r0 + nr], dec_m[r0:r0 + nr]
        for g, p, is_ra in ((gra, pra, True), (gdec, pdec, False)):
            d = (g - p).abs()
            if is_ra:
                d = torch.remainder(g - p + math.pi, 2 * math.pi).sub_(math.pi).abs_()
            bound = _pp_bound(p, a0, is_ra, inf)
            assert torch.isfinite(g).all(), (tag, r0)
            ratio = float((d / bound).max())
            assert ratio <= 1.0, (tag, "ra" if is_ra else "dec", r0, ratio)
            worst["pp"] = max(worst["pp"], ratio)
            worst["pp_abs"] = max(worst["pp_abs"], float(d.max()))
        # (2) the oracle, with the bound test_gnomonic_wide_fields_on_device applies to the scattered evaluator
        ic, jc = ii.cpu().numpy().ravel(), jj.cpu().numpy().ravel()
        era, edec = O.pix2sky_tan(wcs, ic, jc)
        tol = 4e-16 * np.abs(era) + 2e-15 / np.maximum(np.cos(edec), 1e-6)
        gr, gd = gra.cpu().numpy().ravel(), gdec.cpu().numpy().ravel()
        e1, e2 = _wrap(gr - era), np.abs(gd - edec)
        assert (e1 < tol).all() and (e2 < 4e-16 * np.abs(edec) + 2e-15 / np.maximum(np.cos(edec), 1e-6)).all(), (tag, r0)
        worst["oracle"] = max(worst["oracle"], float(e1.max()), float(e2.max()))
    # (3) long double on sampled pixels: every 61st row, and the tile-edge columns of 200 random rows
    rng = np.random.default_rng(nx * 7 + ny)
    rows = np.arange(0, ny, 61)
    jj, ii = np.meshgrid(rows + 1.0, np.arange(1, nx + 1, dtype=float), indexing="ij")
    edge = np.array([0, 1, 7, 8, 63, 64, 119, 120, 126, 127])
    ecols = (np.arange(0, nx, TG_W)[:, None] + edge[None, :]).ravel()
    ecols = ecols[ecols < nx]
    rrows = rng.integers(0, ny, 200)
    jj2, ii2 = np.meshgrid(rrows + 1.0, ecols + 1.0, indexing="ij")
    ii, jj = np.concatenate([ii.ravel(), ii2.ravel()]), np.concatenate([jj.ravel(), jj2.ravel()])
    ri, rj = (ii - 1).astype(np.int64), (jj - 1).astype(np.int64)
    gr = ra_m.cpu().numpy()[rj, ri]
    gd = dec_m.cpu().numpy()[rj, ri]
    tra, tdec = _tan_pix2sky_ld(wcs, ii, jj)
    tra64, tdec64 = tra.astype(float), tdec.astype(float)
    tol = 4e-16 * np.abs(tra64) + 2e-15 / np.maximum(np.cos(tdec64), 1e-6)
    e1 = _wrap((gr - tra).astype(float))
    e2 = np.abs((gd - tdec).astype(float))
    # DEC: the per-point bound of tests/test_gpu_gnomonic_accuracy.py for interpolated pixels (no 1 / cos(DEC))
    _, _, _, b_dec = G.pix2sky_bounds(wcs, ii, jj, grid=True)
    assert (e1 < tol).all() and (e2 <= b_dec).all(), (tag, float((e2 / b_dec).max()))
    worst["ld"] = max(float(e1.max()), float(e2.max()))
    print("posmap %s %s: grid vs per-pixel max %.3g of the bound (%.3g rad), vs oracle %.3g rad, vs long double %.3g rad"
          % (tag, shape, worst["pp"], worst["pp_abs"], worst["oracle"], worst["ld"]))
    return ra_m, dec_m, worst


def test_posmap_grid_bench_patch_per_pixel(pj, O, dev):
    """bench.py's Gnomonic posmap: 8192^2 pixels of 0.5' centred on (40, -25) -- even nx, so k_posmap_tan_grid<true> (16-byte
    stores), and 128 tile rows, so the eight-front deal of tile rows.  Held per pixel (see _check_posmap).
    Measured on the MI355X: grid vs per-pixel 0.89 of its bound (5.6e-16 rad), 8.9e-16 rad from the oracle, 4.4e-16 from long double."""
    _need_longdouble()
    n = 8192
    wcs = pj.Gnomonic((-0.5 / 60, 0.5 / 60), (n / 2 + 0.5, n / 2 + 0.5), (40.0, -25.0))
    assert _grid_taken(wcs, (n, n), n) and -(-n // TG_ROWS) >= 32
    _check_posmap(pj, O, dev, (n, n), wcs, tag="bench 8192^2")


def test_posmap_grid_odd_partial_tiles_and_windows(pj, O, dev):
    """4099 x 2113 with cdelt = (-0.5', 0.5'): odd nx (k_posmap_tan_grid<false>), a partial last tile column (3 columns) and
    tile row (1 row); 34 tile rows dealt to 8 fronts of 5 (the last part idle).  Windows (row0, nrows) of the grid form are
    bit-identical to the same rows of the full map (the form is row-local); a 7-row window takes the per-pixel kernel and is held
    to the per-pixel bound instead.  Passes on the MI355X."""
    _need_longdouble()
    shape = (4099, 2113)
    wcs = pj.Gnomonic((-0.5 / 60, 0.5 / 60), (2050.0, 1000.5), (123.0, 31.0))
    assert _grid_taken(wcs, shape, shape[1]) and -(-shape[1] // TG_ROWS) == 34
    ra, dec, _ = _check_posmap(pj, O, dev, shape, wcs, tag="odd 4099x2113")
    ra, dec = ra.cpu().numpy(), dec.cpu().numpy()
    for n in (8, 63, 64, 65, 130):
        for r0 in (0, 64, 100, 1983, shape[1] - n):
            wr, wd = pj.posmap(shape, wcs, device=dev, row0=r0, nrows=n)
            assert bits_equal(wr.data.cpu().numpy(), ra[r0:r0 + n]) and bits_equal(wd.data.cpu().numpy(), dec[r0:r0 + n]), (n, r0)
    inf = torch.tensor(math.inf, dtype=torch.float64, device=dev)
    for r0 in (0, 77, shape[1] - 7):
        wr, wd = pj.posmap(shape, wcs, device=dev, row0=r0, nrows=7)
        jj = torch.arange(r0 + 1, r0 + 8, dtype=torch.float64, device=dev)[:, None].expand(7, shape[0]).contiguous()
        ii = torch.arange(1, shape[0] + 1, dtype=torch.float64, device=dev)[None, :].expand(7, shape[0]).contiguous()
        pra, pdec = pj.pix2sky((shape, wcs), ii, jj, safe=False)
        a0 = wcs.crval[0] * math.pi / 180
        for g, p, is_ra in ((wr.data, pra, True), (wd.data, pdec, False)):
            assert ((g - p).abs() <= _pp_bound(p, a0, is_ra, inf)).all(), r0


@pytest.mark.parametrize("res_arcmin", [1.06, 1.09])
def test_posmap_grid_pays_threshold(pj, O, dev, res_arcmin):
    """Pixels of 1.06' (a tile spans 0.0395 rad: the grid kernel) and 1.09' (0.0406 rad, beyond grid_pays' 0.04: the per-pixel
    kernel), both held to the same per-pixel bounds.  Passes on the MI355X."""
    _need_longdouble()
    shape = (1030, 700)
    wcs = pj.Gnomonic((-res_arcmin / 60, res_arcmin / 60), (515.5, 350.5), (300.0, -48.0))
    assert _grid_taken(wcs, shape, shape[1]) == (res_arcmin < 1.07)
    _check_posmap(pj, O, dev, shape, wcs, tag="%.2f'" % res_arcmin)


def _row_fallback_expected(wcs, shape):
    """Per map row and tile column: does the row fail the grid form's preconditions (pxl_tan.h tg_delta: D <= 0, or a
    small-angle argument above 1/16 at a node column)?  Host arithmetic in double, from the row geometry alone."""
    nx, ny = shape
    uos = wcs.unit * wcs.cdelt[0]
    d0 = wcs.crval[1] * math.pi / 180
    sd0, cd0 = math.sin(d0), math.cos(d0)
    Y = (wcs.crpix[1] - np.arange(1, ny + 1)) * uos
    den, num = sd0 * Y + cd0, sd0 - cd0 * Y
    ntx = -(-nx // TG_W)
    fail = np.zeros((ny, ntx), bool)
    h = (TG_W - 1.0) / (TG_NODES - 1)
    for tx in range(ntx):
        Xa = (wcs.crpix[0] - (tx * TG_W + TG_W / 2 + 1)) * uos
        rho_a = np.sqrt(Xa * Xa + den * den)
        for k in range(TG_NODES):
            dX = (k * h - TG_W / 2) * uos
            X = Xa - dX
            dot = X * Xa + den * den
            s = den * dX / dot
            rho = np.sqrt(X * X + den * den)
            s2 = num * dX * (Xa + X) / ((rho_a + rho) * (rho * rho_a + num * num))
            fail[:, tx] |= ~(den > 0) | ~(dot > 0) | (np.abs(s) > TG_SMAX) | (np.abs(s2) > TG_SMAX)
    return fail


def test_posmap_grid_mixed_rows_near_pole(pj, O, dev):
    """1' pixels centred at dec 72 (cos d0 = 0.31: the grid kernel is taken) on a map that reaches 1448 rows above the centre,
    so the pole (1117 rows up) and the rows around it lie inside: there a tile's rows split between the interpolant and the
    per-pixel fallback (a mixed okmask; rows whose small-angle argument exceeds 1/16 or beyond the pole, where D <= 0).
    Passes on the MI355X."""
    _need_longdouble()
    shape = (1024, 2048)
    wcs = pj.Gnomonic((-1.0 / 60, 1.0 / 60), (512.5, 600.5), (10.0, 72.0))
    assert _grid_taken(wcs, shape, shape[1])
    pole_row = 600.5 + math.tan(18 * DEG) / ARCMIN
    assert 1 < pole_row < shape[1]
    fail = _row_fallback_expected(wcs, shape)
    mixed = 0
    for ty in range(-(-shape[1] // TG_ROWS)):
        f = fail[ty * TG_ROWS:(ty + 1) * TG_ROWS]
        mixed += int((f.any(axis=0) & ~f.all(axis=0)).sum())
    assert fail.any() and (~fail).any() and mixed > 0, mixed
    _check_posmap(pj, O, dev, shape, wcs, tag="pole 72")


# ---- B. k_reproject_generic_tiled3 coordinates, pixel by pixel ---------------------------------------

def _ramp(shape, dev, dtype=torch.float64):
    """plane 0: the 1-based column index, plane 1: the 1-based row index.  Bilinear interpolation reproduces an affine field, so
    in every interior cell the output planes ARE the source coordinates the kernel used."""
    nx, ny = shape
    r = torch.empty((2, ny, nx), dtype=dtype, device=dev)
    r[0].copy_(torch.arange(1, nx + 1, dtype=dtype, device=dev)[None, :].expand(ny, nx))
    r[1].copy_(torch.arange(1, ny + 1, dtype=dtype, device=dev)[:, None].expand(ny, nx))
    return r


def _ref_coords(pj, src_shape, src_wcs, out_wcs, ii, jj):
    """long-double source coordinates of output pixel centres (ii, jj), the sky angles, and cos c (1 for a CAR source)"""
    p2s = _tan_pix2sky_ld if isinstance(out_wcs, pj.Gnomonic) else _car_pix2sky_ld
    ra, dec = p2s(out_wcs, ii, jj)
    if isinstance(src_wcs, pj.Gnomonic):
        x, y, cosc = _tan_sky2pix_ld(src_wcs, ra, dec)
    else:
        x, y = _car_sky2pix_ld(src_wcs, src_shape, ra, dec)
        cosc = np.ones_like(x)
    return x, y, ra, dec, cosc


def _src_pix_rad(pj, wcs):
    if isinstance(wcs, pj.Gnomonic):
        return abs(wcs.cdelt[0] * wcs.unit), abs(wcs.cdelt[0] * wcs.unit)
    return abs(wcs.cdelt[0] * wcs.unit), abs(wcs.cdelt[1] * wcs.unit)


def _check_ramp(pj, src_shape, src_wcs, out_wcs, got, rows, exact_path, tag):
    """got: (2, nrows_sampled, nxo) output planes of a ramp source at output rows `rows` (0-based).  Returns
    (max error / bound over interior cells, masks of interior and invisible pixels, reference x)."""
    nxo = got.shape[2]
    jj, ii = np.meshgrid(np.asarray(rows) + 1.0, np.arange(1, nxo + 1, dtype=float), indexing="ij")
    x, y, ra, dec, cosc = _ref_coords(pj, src_shape, src_wcs, out_wcs, ii, jj)
    nx, ny = src_shape
    m = 1e-6
    interior = (cosc > 1e-6) & (x >= 1 + m) & (x < nx - m) & (y >= 1 + m) & (y < ny - m)
    px, py = _src_pix_rad(pj, src_wcs)
    ang = np.maximum(np.abs(ra), np.abs(dec)).astype(float)
    dang = 4 * np.spacing(ang)
    worst = 0.0
    for plane, ref, pix in ((0, x, px), (1, y, py)):
        # the coordinate is crpix + offset: its roundings are ulp of the larger of the two magnitudes
        r64 = ref.astype(float)
        mag = np.maximum(np.abs(r64), np.abs(r64 - src_wcs.crpix[plane]))
        bound = 8 * np.spacing(mag) + dang / pix + (0.0 if exact_path else PXL_TILED_TOL)
        err = np.abs((got[plane] - ref).astype(float))
        ratio = np.where(interior, err / bound, 0.0)
        assert np.isfinite(got[plane][interior]).all(), tag
        k = int(np.argmax(ratio))
        assert ratio.max() <= 1.0, (tag, plane, float(ratio.max()), float(err.ravel()[k]), float(bound.ravel()[k]))
        worst = max(worst, float(ratio.max()))
    invisible = cosc < -1e-6
    assert (got[:, invisible] == 0).all(), tag
    return worst, interior, invisible, x


def _run_generic(pj, dev, src, src_wcs, out_shape, out_wcs, how, monkeypatch=None):
    """one output of the reprojection of map `src` through the one-shot entry ('tiled' / 'exact') or a plan ('plan')"""
    m = pj.Enmap(src, src_wcs)
    nxo, nyo = out_shape
    out = pj.Enmap(torch.full((src.shape[0], nyo, nxo), float("nan"), dtype=torch.float64, device=dev), out_wcs)
    if how == "plan":
        plan = pj.GenericReprojectPlan((src.shape[2], src.shape[1]), src_wcs, out_shape, out_wcs, device=dev)
        pj.reproject(m, out_shape, out_wcs, out=out, plan=plan)
        tiles = plan.tiles()
        plan.close()
    else:
        if how == "exact":
            monkeypatch.setenv("PXL_GENERIC_EXACT", "1")
        try:
            pj.reproject(m, out_shape, out_wcs, out=out)
        finally:
            if how == "exact":
                monkeypatch.delenv("PXL_GENERIC_EXACT")
        tiles = None
    torch.cuda.synchronize()
    return out.data, tiles


def _smooth(shape):
    nx, ny = shape
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    return (np.sin(0.01 * xx) * np.cos(0.013 * yy))[None]


def _ramp_case(pj, O, dev, src_shape, src_wcs, out_shape, out_wcs, want, monkeypatch, tag, rows=None, oracle_excluded=True,
               min_interior=0.5):
    """The output planes of a ramp source through the tiled one-shot entry, a plan and the per-pixel path, each against the
    long-double coordinates; the excluded pixels (edges, the RA seam of a periodic source, invisible) separately.
    `want` in {"none", "some", "all"}: the plan's count of per-pixel tiles.  Returns (worst ratio, (exact, total))."""
    src = _ramp(src_shape, dev)
    nxo, nyo = out_shape
    rows = np.arange(nyo) if rows is None else np.asarray(rows)
    res = {}
    for how in ("tiled", "plan", "exact"):
        got, tiles = _run_generic(pj, dev, src, src_wcs, out_shape, out_wcs, how, monkeypatch)
        res[how] = got.cpu().numpy()[:, rows]
        if tiles is not None:
            ex, tot = plan_tiles = tiles
            assert tot == -(-nxo // 128) * -(-nyo // 32)
            assert {"some": 0 < ex < tot, "none": ex == 0, "all": ex == tot}[want], (tag, ex, tot)
    assert bits_equal(res["plan"], res["tiled"]), tag
    worst = {}
    for how in ("tiled", "exact"):
        worst[how], interior, invisible, xref = _check_ramp(pj, src_shape, src_wcs, out_wcs, res[how], rows, how == "exact",
                                                            tag + " " + how)
    assert interior.mean() > min_interior, (tag, interior.mean())      # the case tests what it is meant to
    excluded = ~interior & ~invisible
    if oracle_excluded and excluded.any():
        # the ramp is not affine across the seam or the edges: the excluded pixels on a smooth map against the oracle
        sm = _smooth(src_shape)
        got = pj.reproject(pj.Enmap(to_dev(sm[0], dev), src_wcs), out_shape, out_wcs).data.cpu().numpy()[rows]
        exp = O.reproject_generic(src_wcs, int(isinstance(src_wcs, pj.Gnomonic)), (src_shape[0], src_shape[1], 1), sm, out_wcs,
                                  int(isinstance(out_wcs, pj.Gnomonic)), out_shape)[0][rows]
        same_nan = np.isnan(got) == np.isnan(exp)
        assert same_nan[excluded].all(), tag
        ok = excluded & ~np.isnan(exp)
        assert (np.abs(got[ok] - exp[ok]) < 1e-9).all(), (tag, np.abs(got[ok] - exp[ok]).max())
    print("ramp %s: tiled max %.3g of its bound, per-pixel %.3g; tiles %s; excluded %d, invisible %d"
          % (tag, worst["tiled"], worst["exact"], plan_tiles, int(excluded.sum()), int(invisible.sum())))
    return worst, plan_tiles


def _strip_05():
    """a declination strip of the 0.5' full-sky CAR map (full rings: periodic)"""
    import pixell_jl_amd as pj
    fshape, fwcs = pj.fullsky_geometry(2 * math.pi / 43200)
    return pj.slice_geometry(fshape, fwcs, None, (10801 - 700, 10801 + 700))


def test_tiled_coords_car_to_tan_inside_and_seam(pj, O, dev, monkeypatch):
    """CAR -> TAN from a periodic 0.5' strip: a patch well inside the map (no per-pixel tiles) and one that straddles the RA seam
    (the tiles across the rewind jump are evaluated per pixel).  Per interior pixel: tiled <= PXL_TILED_TOL + 8 ulp(x) +
    4 ulp(angle) / pixel, per-pixel path the same without PXL_TILED_TOL.  Measured on the MI355X: inside 0.32 of the bound
    tiled, 0.55 per pixel, 0 of 96 tiles per pixel; seam 0.51 tiled, 0.17 per pixel, 16 of 96 tiles per pixel."""
    _need_longdouble()
    fshape, fwcs = _strip_05()
    inner = ((700, 500), pj.Gnomonic((0.5 / 60, 0.5 / 60), (350.5, 250.5), (40.0, -1.0)))
    seam = ((700, 500), pj.Gnomonic((0.5 / 60, 0.5 / 60), (350.5, 250.5), (179.9, 0.3)))
    _ramp_case(pj, O, dev, fshape, fwcs, *inner, "none", monkeypatch, "car->tan inside")
    _ramp_case(pj, O, dev, fshape, fwcs, *seam, "some", monkeypatch, "car->tan seam")


def test_tiled_coords_coarse(pj, O, dev, monkeypatch):
    """40' pixels: every tile fails its check and is evaluated per pixel.  Measured on the MI355X: tiled 0.0037 of its bound,
    per-pixel 0.39; 10 of 10 tiles per pixel."""
    _need_longdouble()
    fshape, fwcs = pj.fullsky_geometry(2 * math.pi / 2160)           # 10' full sky
    coarse = ((200, 150), pj.Gnomonic((40.0 / 60, 40.0 / 60), (100.5, 75.5), (10.0, 3.0)))
    _ramp_case(pj, O, dev, fshape, fwcs, *coarse, "all", monkeypatch, "40'")


@pytest.mark.xfail(strict=True, reason="the tiled interpolant's twelve check points sample its error and do not bound it: at 1.2' "
                                       "pixels a pixel between them lies 1.13e-10 pixel from the exact coordinate (PXL_TILED_TOL "
                                       "= 1e-10); a margin on the check (TOL / 2) sends noise-limited tiles of fine maps per "
                                       "pixel and made the 0.5' mosaic 3x slower, so the check needs another design")
def test_tiled_coords_partial(pj, O, dev, monkeypatch):
    """The first pixel size between 1' and 8' at which only part of the tiles pass their check: the two kinds of tile side by
    side in one output, held per pixel.  Measured on the MI355X: the first such size is 1.2', where one pixel of a passing tile
    lies 1.128e-10 pixel off against a bound of 1.103e-10 (1.02 of it)."""
    _need_longdouble()
    fshape, fwcs = pj.fullsky_geometry(2 * math.pi / 21600)          # 1' full sky
    found = None
    for res in [1.0 + 0.05 * k for k in range(20)] + [2.0, 3.0, 4.0, 6.0, 8.0]:
        oshape = (512, 384)
        owcs = pj.Gnomonic((res / 60, res / 60), (256.5, 192.5), (60.0, 20.0))
        plan = pj.GenericReprojectPlan(fshape, fwcs, oshape, owcs, device=dev)
        ex, tot = plan.tiles()
        plan.close()
        if 0 < ex < tot:
            found = (res, oshape, owcs)
            break
    assert found is not None, "no pixel size between 1' and 8' with part of the tiles per pixel"
    res, oshape, owcs = found
    _ramp_case(pj, O, dev, fshape, fwcs, oshape, owcs, "some", monkeypatch, "%g' partial" % res, oracle_excluded=False)


def test_tiled_coords_tan_sources(pj, O, dev, monkeypatch):
    """TAN -> CAR and TAN -> TAN from a 0.5' Gnomonic source, and TAN -> TAN onto 40' pixels that reach beyond the source's
    horizon (invisible pixels give exactly 0).  Measured on the MI355X: TAN -> CAR 0.033 of the bound tiled, 0.20 per pixel (0 of
    380 tiles per pixel); TAN -> TAN 0.034 / 0.24 (0 of 80); horizon 0.0016 / 0.55 (12 of 12)."""
    _need_longdouble()
    sshape = (2000, 1600)
    swcs = pj.Gnomonic((-0.5 / 60, 0.5 / 60), (1000.5, 800.5), (40.0, -1.0))
    cshape, cwcs = pj.geometry([[45 * DEG, 35 * DEG], [-6 * DEG, 4 * DEG]], 0.5 * ARCMIN)
    cshape = (cshape[0], cshape[1])
    _ramp_case(pj, O, dev, sshape, swcs, cshape, cwcs, "none", monkeypatch, "tan->car")
    _ramp_case(pj, O, dev, sshape, swcs, (600, 500), pj.Gnomonic((0.6 / 60, 0.6 / 60), (300.0, 250.0), (40.3, -1.2)),
               "none", monkeypatch, "tan->tan")
    # far side: a 40' patch centred 80 degrees away sees the source plane's horizon (cos c <= 0 -> 0, per-pixel tiles there)
    w, tiles = _ramp_case(pj, O, dev, (400, 400), pj.Gnomonic((-30.0 / 60, 30.0 / 60), (200.5, 200.5), (0.0, 0.0)),
                          (256, 192), pj.Gnomonic((40.0 / 60, 40.0 / 60), (128.5, 96.5), (80.0, 0.0)), "all", monkeypatch,
                          "tan->tan horizon", min_interior=0.2)
    assert w["exact"] <= 1.0


def test_tiled_nonfinite_source_gives_nan(pj, dev):
    """a NaN in the source reaches exactly the output pixels whose four taps include it; every other pixel keeps its bits"""
    fshape, fwcs = _strip_05()
    oshape, owcs = (700, 500), pj.Gnomonic((0.5 / 60, 0.5 / 60), (350.5, 250.5), (40.0, -1.0))
    src = _ramp(fshape, dev)
    base = pj.reproject(pj.Enmap(src, fwcs), oshape, owcs).data.cpu().numpy()
    x, y = base[0], base[1]
    ci, cj = int(x[250, 350]), int(y[250, 350])                   # a source pixel (1-based) under the patch centre
    src[:, cj - 1, ci - 1] = float("nan")
    got = pj.reproject(pj.Enmap(src, fwcs), oshape, owcs).data.cpu().numpy()
    touch = (np.floor(x) >= ci - 1) & (np.floor(x) <= ci) & (np.floor(y) >= cj - 1) & (np.floor(y) <= cj)
    assert touch.sum() > 0
    assert np.isnan(got[:, touch]).all()
    assert bits_equal(got[:, ~touch], base[:, ~touch])


def test_tiled_coords_large_source_64bit_offsets(pj, dev, monkeypatch):
    """A declination strip of the 0.25' full-sky CAR map, rows 1..26000: 86400 x 26000 = 2.25e9 elements per plane, beyond 2^31,
    so k_reproject_generic_tiled3 takes its 64-bit offset branch.  A 0.25' TAN patch around dec 16 (away from the seam) reads
    rows above 24 856, where the element offsets exceed 2^31.  Both ramp planes live on the device (36 GB); sampled rows are
    held to the per-pixel bound.  Measured on the MI355X: 0.55 of the bound, 0 tiles per pixel."""
    _need_longdouble()
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 48 * 2 ** 30:
        pytest.skip("needs 48 GiB of free device memory for the 2 x 2.25e9-element ramp source, %.1f GiB free" % (free / 2 ** 30))
    fshape, fwcs = pj.fullsky_geometry(2 * math.pi / 86400)
    sshape, swcs = pj.slice_geometry(fshape, fwcs, None, (1, 26000))
    sshape = (sshape[0], sshape[1])
    assert sshape[0] * sshape[1] > 2 ** 31
    oshape, owcs = (2048, 1024), pj.Gnomonic((0.25 / 60, 0.25 / 60), (1024.5, 512.5), (100.0, 16.0))
    rows = np.concatenate([np.arange(0, 1024, 7), [1023]])
    src = _ramp(sshape, dev)
    try:
        res = {}
        for how in ("tiled", "plan"):
            got, tiles = _run_generic(pj, dev, src, swcs, oshape, owcs, how, monkeypatch)
            res[how] = got.cpu().numpy()[:, rows]
            if tiles is not None:
                assert tiles[0] == 0, tiles
        assert bits_equal(res["plan"], res["tiled"])
        worst, interior, invisible, _ = _check_ramp(pj, sshape, swcs, owcs, res["tiled"], rows, False, "0.25' strip")
        assert interior.all()
        assert res["tiled"][1].min() > 24857           # every tap row lies beyond the 2^31-element offset
        print("ramp 0.25' strip (2.25e9 elements): tiled max %.3g of its bound" % worst)
    finally:
        del src
        torch.cuda.empty_cache()


# ---- C. one-shot calls on several streams and threads --------------------------------------------------

def _race_cases(pj):
    fshape, fwcs = pj.fullsky_geometry(2 * math.pi / 43200)
    fshape, fwcs = pj.slice_geometry(fshape, fwcs, None, (10801 - 1300, 10801 + 1300))
    big = ((4096, 2048), pj.Gnomonic((0.5 / 60, 0.5 / 60), (2048.5, 1024.5), (179.0, 0.0)))
    small = [((256 + 32 * k, 160), pj.Gnomonic((0.5 / 60, 0.5 / 60), (100.5 + 10 * k, 80.5), (179.95 - 0.05 * k, 1.0 - 0.3 * k)))
             for k in range(8)]
    return (fshape, fwcs), big, small


def test_one_shot_concurrent_streams_and_threads(pj, dev):
    """Every one-shot generic call counts its per-pixel tiles in a counter of its own.  A seam-straddling 4096 x 2048 CAR -> TAN
    patch on stream A and eight small seam patches on stream B, with no synchronisation between them, eight rounds, every output
    passed as out= pre-filled with NaN; then four host threads with a stream each.  Every output must carry the bits of the
    serial call (a skipped per-pixel tile would keep its NaN).  With the two-slot counter shared by all calls this failed on the
    MI355X (four outputs of the thread variant differed); with a counter per call it passes."""
    (fshape, fwcs), big, small = _race_cases(pj)
    nx, ny = fshape
    xx = torch.arange(nx, dtype=torch.float64, device=dev)[None, :]
    yy = torch.arange(ny, dtype=torch.float64, device=dev)[:, None]
    m = pj.Enmap(torch.sin(0.01 * xx) * torch.cos(0.013 * yy), fwcs)
    cases = [big] + small
    serial = []
    for oshape, owcs in cases:
        plan = pj.GenericReprojectPlan(fshape, fwcs, oshape, owcs, device=dev)
        ex, tot = plan.tiles()
        plan.close()
        assert 0 < ex, (oshape, owcs.crval)                # every case has per-pixel tiles
        serial.append(pj.reproject(m, oshape, owcs).data.cpu().numpy())
        assert np.isfinite(serial[-1]).all()
    torch.cuda.synchronize()

    def nan_out(k):
        oshape, owcs = cases[k]
        return pj.Enmap(torch.full((oshape[1], oshape[0]), float("nan"), dtype=torch.float64, device=dev), owcs)

    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    bad = []
    for rnd in range(8):
        outs = [None] * len(cases)
        with torch.cuda.stream(sa):
            outs[0] = nan_out(0)
            pj.reproject(m, cases[0][0], cases[0][1], out=outs[0])
        with torch.cuda.stream(sb):
            for k in range(1, len(cases)):
                outs[k] = nan_out(k)
                pj.reproject(m, cases[k][0], cases[k][1], out=outs[k])
        torch.cuda.synchronize()
        bad += [(rnd, k) for k in range(len(cases)) if not bits_equal(outs[k].data.cpu().numpy(), serial[k])]
    assert not bad, bad

    errors, results = [], {}

    def work(t):
        try:
            st = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(st):
                for rnd in range(4):
                    for k in range(t, len(cases), 4):
                        out = nan_out(k)
                        pj.reproject(m, cases[k][0], cases[k][1], out=out)
                        results[(t, rnd, k)] = out
                st.synchronize()
        except Exception as e:                            # pragma: no cover
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    torch.cuda.synchronize()
    bad = [key for key, out in results.items() if not bits_equal(out.data.cpu().numpy(), serial[key[2]])]
    assert len(results) == 4 * len(cases) and not bad, bad


def test_last_tiles_reports_the_call_on_its_stream(pj, dev):
    """pxl_reproject_generic_last_tiles after one-shot calls on one stream: the count of the call just made, as the plan of the
    same geometries reports it."""
    import ctypes as C
    (fshape, fwcs), big, small = _race_cases(pj)
    m = pj.Enmap(torch.zeros((fshape[1], fshape[0]), dtype=torch.float64, device=dev), fwcs)
    lib = pj.load_library()
    inner = ((520, 300), pj.Gnomonic((0.5 / 60, 0.5 / 60), (260.5, 150.5), (40.0, -1.0)))
    for oshape, owcs in [small[0], inner, small[3], big]:
        plan = pj.GenericReprojectPlan(fshape, fwcs, oshape, owcs, device=dev)
        want = plan.tiles()
        plan.close()
        pj.reproject(m, oshape, owcs)
        ex, tot = C.c_int64(), C.c_int64()
        pj._lib.check(lib.pxl_reproject_generic_last_tiles(C.byref(ex), C.byref(tot),
                                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        assert (ex.value, tot.value) == want, (oshape, (ex.value, tot.value), want)
