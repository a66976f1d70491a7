"""Special pixel values for the interpolating kernels: the map builder, the bit-level comparison and a plain numpy restatement
of the bilinear definition R1 (oracle/pixell_oracle.c).  Shared by test_oracle_special_values.py (CPU) and
test_gpu_special_values.py (device).  numpy only.

Kinds (one per test parameter):
  nan, +inf, -inf   the value itself
  mixed_inf         +Inf and -Inf alternating along every placed line (their weighted sum is NaN)
  neg_zero_all      the WHOLE map is +-0.0 with random signs (nothing else is placed)
  neg_zero          -0.0 placed / sprinkled in normal data
  subnormal         5e-324 .. 2e-308 with random signs (Float32 maps: 1e-45 .. 1e-38)
  huge              +-1.7e308 in runs of equal sign (Float32 maps: +-3.4e38 and +-FLT_MAX), so (1 - f) M + f M rounds next to
                    the overflow limit
  sentinel          -1.6375e30
"""
import numpy as np

KINDS = ["nan", "+inf", "-inf", "mixed_inf", "neg_zero_all", "neg_zero", "subnormal", "huge", "sentinel"]
NONFINITE = ("nan", "+inf", "-inf", "mixed_inf")
# Fraction of sprinkled pixels.  A bilinear output reads four taps, so a fraction p of special pixels reaches 1 - (1 - p)^4 of
# the outputs whatever the scale factor: 1.5 % gives 5.9 %, which is what the 5 % floor of the non-vacuity checks needs
# (1 % gives 3.9 %).
SPRINKLE = 0.015


def _values(kind, n, rng, f32):
    """n special values laid along a line: neighbours in the array are neighbours in the map"""
    k = np.arange(n)
    if kind == "nan":
        return np.full(n, np.nan)
    if kind == "+inf":
        return np.full(n, np.inf)
    if kind == "-inf":
        return np.full(n, -np.inf)
    if kind == "mixed_inf":
        return np.where(k % 2 == 0, np.inf, -np.inf)
    if kind in ("neg_zero", "neg_zero_all"):
        return np.full(n, -0.0)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if kind == "subnormal":
        lo, hi = (1e-45, 1e-38) if f32 else (5e-324, 2e-308)
        v = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
        v[::3] = lo
        v[1::3] = hi
        v = v.astype(np.float32).astype(np.float64) if f32 else v
        assert (v != 0).all()
        return sign * v
    if kind == "huge":
        run = np.where((k // 8) % 2 == 0, 1.0, -1.0)                  # runs of eight equal signs
        if f32:
            m = np.where(k % 3 == 0, float(np.finfo(np.float32).max), float(np.float32(3.4e38)))
            return run * m
        return run * 1.7e308
    if kind == "sentinel":
        return np.full(n, -1.6375e30)
    raise ValueError(kind)


def special_map(kind, shape, nc=1, seed=0, f32=False, mode="placed", rows=(), cols=()):
    """(nc, ny, nx) map and the boolean mask of its special pixels.  shape = (nx, ny).
    placed:     the four corners, the first and last row, the first and last column (the seam pair of a periodic map), one
                interior row and one interior column, plus the 0-based `rows` and `cols` the caller adds (window edges, source
                columns under output-tile boundaries);
    sprinkled:  a seeded SPRINKLE of all pixels."""
    nx, ny = int(shape[0]), int(shape[1])
    rng = np.random.default_rng(seed)
    m = rng.normal(size=(nc, ny, nx))
    mask = np.zeros((ny, nx), bool)
    if kind == "neg_zero_all":
        m = np.where(rng.random((nc, ny, nx)) < 0.5, -0.0, 0.0)
        mask[:] = True
    elif mode == "sprinkled":
        mask = rng.random((ny, nx)) < SPRINKLE
    else:
        assert mode == "placed"
        for r in [0, ny - 1, ny // 2 + 1] + [int(r) for r in rows]:
            if 0 <= r < ny:
                mask[r, :] = True
        for c in [0, nx - 1, nx // 3] + [int(c) for c in cols]:
            if 0 <= c < nx:
                mask[:, c] = True
    if kind != "neg_zero_all":
        for c in range(nc):
            # rows first, then columns: values are adjacent along whichever line was written last
            plane = m[c]
            for r in np.flatnonzero(mask.all(axis=1)):
                plane[r, :] = _values(kind, nx, rng, f32)
            for col in np.flatnonzero(mask.all(axis=0)):
                plane[:, col] = _values(kind, ny, rng, f32)
            rest = mask & ~mask.all(axis=1)[:, None] & ~mask.all(axis=0)[None, :]
            plane[rest] = _values(kind, int(rest.sum()), rng, f32)
    if f32:
        m = m.astype(np.float32)
    return m, mask


# ---- comparison ----------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _nearest_special(v):
    v = float(v)
    if np.isnan(v):
        return "nan"
    if np.isinf(v):
        return "+inf" if v > 0 else "-inf"
    if v == 0:
        return "-0.0" if np.signbit(v) else "+0.0"
    a = abs(v)
    if a < 2.3e-308:
        return "subnormal(f64)"
    if a < 1.2e-38:
        return "subnormal(f32) / tiny"
    if a > 1e307:
        return "huge(f64)"
    if a > 1e37:
        return "sentinel" if abs(v + 1.6375e30) < 1e24 else "huge(f32)"
    if abs(v + 1.6375e30) < 1e24:
        return "sentinel"
    return "ordinary"


def same(got, expect):
    """(ok, message).  NaN in exactly the same positions; every other element equal as bits (sign of zero, +-Inf and
    subnormals count).  Sign and payload of a NaN are not compared.  Float64 or Float32, both arrays of the same type."""
    got, expect = np.asarray(got), np.asarray(expect)
    if got.shape != expect.shape or got.dtype != expect.dtype or got.dtype not in (np.float64, np.float32):
        return False, "shape / dtype: %s %s against %s %s" % (got.shape, got.dtype, expect.shape, expect.dtype)
    ng, ne = np.isnan(got), np.isnan(expect)
    zero = got.dtype.type(0)
    bad = (ng != ne) | (_bits(np.where(ng, zero, got)) != _bits(np.where(ne, zero, expect)))
    if not bad.any():
        return True, ""
    idx = np.argwhere(bad)
    width = 16 if got.dtype == np.float64 else 8
    lines = ["%d of %d elements differ" % (int(bad.sum()), bad.size)]
    for ix in idx[:6]:
        ix = tuple(int(v) for v in ix)
        g, e = got[ix], expect[ix]
        lines.append("  %s: got %r (0x%0*x, %s), expected %r (0x%0*x, %s)"
                     % (ix, float(g), width, int(_bits(np.array([g]))[0]) & ((1 << 4 * width) - 1), _nearest_special(g),
                        float(e), width, int(_bits(np.array([e]))[0]) & ((1 << 4 * width) - 1), _nearest_special(e)))
    return False, "\n".join(lines)


def assert_same(got, expect, tag):
    ok, msg = same(got, expect)
    assert ok, "%s: %s" % (tag, msg)


# ---- R1 in plain numpy ---------------------------------------------------------------------------------------------------
def _tap(planes, nx, ny, row0, periodic, i, j):
    """planes (nc, nrows, nx) resident rows [row0, row0 + nrows); i, j 1-based int64 arrays -> (nc,) + shape.  A tap outside
    the map (rows; columns of a non-periodic map) or outside the resident window is the VALUE 0.0."""
    nrows = planes.shape[1]
    jr = j - 1 - row0
    ok = (j >= 1) & (j <= ny) & (jr >= 0) & (jr < nrows)
    if periodic:
        ii = (i - 1) % nx
    else:
        ok = ok & (i >= 1) & (i <= nx)
        ii = i - 1
    ok = np.broadcast_to(ok, np.broadcast(ii, jr).shape)
    if nrows == 0:
        return np.zeros((planes.shape[0],) + ok.shape)
    v = planes[:, np.clip(jr, 0, nrows - 1), np.clip(ii, 0, nx - 1)]
    return np.where(ok[None], v, 0.0)


def r1_bilerp(planes, shape, x, y, periodic, row0=0):
    """The comment block "R1" of oracle/pixell_oracle.c: i0 = floor(x), fx = x - i0, j0 = floor(y), fy = y - j0,
    v = (1-fy)*((1-fx)*m[i0,j0] + fx*m[i1,j0]) + fy*((1-fx)*m[i0,j1] + fx*m[i1,j1]); a non-finite x or y gives NaN.
    x, y broadcast against each other; planes are Float64 (nc, nrows, nx)."""
    nx, ny = int(shape[0]), int(shape[1])
    planes = np.asarray(planes, dtype=np.float64)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    fin = np.isfinite(x) & np.isfinite(y)
    xs, ys = np.where(np.isfinite(x), x, 1.0), np.where(np.isfinite(y), y, 1.0)
    fi, fj = np.floor(xs), np.floor(ys)
    fx, fy = xs - fi, ys - fj
    lim = 2.0 ** 40                                       # far outside any map: every tap reads 0 either way
    i0, j0 = np.clip(fi, -lim, lim).astype(np.int64), np.clip(fj, -lim, lim).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a, b = _tap(planes, nx, ny, row0, periodic, i0, j0), _tap(planes, nx, ny, row0, periodic, i0 + 1, j0)
        c, d = _tap(planes, nx, ny, row0, periodic, i0, j0 + 1), _tap(planes, nx, ny, row0, periodic, i0 + 1, j0 + 1)
        top = (1 - fx) * a + fx * b
        bot = (1 - fx) * c + fx * d
        v = (1 - fy) * top + fy * bot
    return np.where(fin[None] if fin.ndim else fin, v, np.nan)


def r1_reproject(O, wcs_in, shape_in, src, wcs_out, shape_out, src_row0=0, dst_row0=0, dst_nrows=None):
    """src (nc, src_nrows, nx) -> (nc, dst_nrows, nxo): R1 at the oracle's coordinate tables (pinned elsewhere)."""
    xs, ys = O.reproject_tables(wcs_in, shape_in, wcs_out, shape_out)
    dst_nrows = shape_out[1] - dst_row0 if dst_nrows is None else dst_nrows
    ys = ys[dst_row0:dst_row0 + dst_nrows]
    per = O.is_periodic(wcs_in, shape_in[0])
    return r1_bilerp(src, shape_in, xs[None, :], ys[:, None], per, src_row0)


def r1_sample(O, wcs, shape, src, sky, src_row0=0):
    """src (nc, src_nrows, nx), sky (n, 2) -> (nc, n): R1 at sky2pix!(safe=true) of the oracle (the reciprocal form)."""
    pix = O.sky2pix(wcs, shape, sky, safe=True, form=O.FORM_RECIP)
    return r1_bilerp(src, shape, pix[:, 0], pix[:, 1], O.is_periodic(wcs, shape[0]), src_row0)


def to_f32(a):
    """ndarray.astype(np.float32) of a Float64 result: overflow to +-Inf is intended"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32)


def zero_weight_special_taps(xs, ys, mask, periodic, src_row0=0, src_nrows=None):
    """Number of output pixels that read a special in-map, resident tap with a weight of exactly zero: the right column of a cell
    with fx == 0 or the lower row of a cell with fy == 0 (from the oracle's coordinate tables)."""
    ny, nx = mask.shape
    src_nrows = ny - src_row0 if src_nrows is None else src_nrows
    res = np.zeros(ny, bool)
    res[src_row0:src_row0 + src_nrows] = True
    m = mask & res[:, None]
    i0, j0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    fx0, fy0 = (xs - np.floor(xs)) == 0, (ys - np.floor(ys)) == 0

    def col(i):
        ok = np.ones(len(i), bool) if periodic else (i >= 1) & (i <= nx)
        return (i - 1) % nx if periodic else np.clip(i - 1, 0, nx - 1), ok

    def row(j):
        return np.clip(j - 1, 0, ny - 1), (j >= 1) & (j <= ny)
    n = 0
    for jj in (j0, j0 + 1):                                # right-hand taps of cells with fx == 0
        r, rok = row(jj)
        c, cok = col(i0 + 1)
        n += int((m[np.ix_(r, c)] & rok[:, None] & (cok & fx0)[None, :]).sum())
    for ii in (i0, i0 + 1):                                # lower taps of cells with fy == 0
        r, rok = row(j0 + 1)
        c, cok = col(ii)
        n += int((m[np.ix_(r, c)] & (rok & fy0)[:, None] & cok[None, :]).sum())
    return n


# ---- the geometries of the CAR -> CAR tests (shared by the CPU and the device file) -------------------------------------------
def _shifted(wcs, dx, dy):
    return type(wcs)(wcs.cdelt, (wcs.crpix[0] + dx, wcs.crpix[1] + dy), wcs.crval, wcs.unit)


def car_cases(pj):
    """name -> (gin, gout, mode).  768 columns: wide enough that a periodic source takes the LDS-DMA kernel in Float64 (slot of
    262 columns at equal resolution) and in Float32 (520).  `placed` cases have integer pixel offsets (weights exactly 0 or 1)."""
    DEG = np.pi / 180
    fs = pj.fullsky_geometry(2 * np.pi / 768)
    assert fs[0] == (768, 385)
    (nx, ny), w = fs
    fine = pj.fullsky_geometry(2 * np.pi / 1536)
    sub = pj.slice_geometry(fs[0], w, (201, 601), (101, 300))                   # 401 x 200, odd nx, not periodic
    odd_out = pj.slice_geometry(fs[0], w, (1, 767), None)                        # 767 output columns
    dec_flip = type(w)((w.cdelt[0], -w.cdelt[1]), w.crpix, w.crval, w.unit)      # output row j is source row ny + 1 - j
    ra_flip = type(w)((-w.cdelt[0], w.cdelt[1]), (w.crpix[0] + 0.25, w.crpix[1] - 0.25), w.crval, w.unit)
    wide = pj.geometry([[179 * DEG, -179 * DEG], [-60 * DEG, 60 * DEG]], 0.5 * DEG)
    s500, w500 = pj.fullsky_geometry(2 * np.pi / 500)
    # RA centre moved by 100 degrees: the box's rewind jump (RA 180) falls inside the first 256-column tile, not on the map's edge
    fs500 = (s500, type(w500)(w500.cdelt, w500.crpix, (w500.crval[0] + 100.0, w500.crval[1]), w500.unit))
    return {
        "identity": (fs, fs, "placed"),
        "integer_shift": (fs, (fs[0], _shifted(w, 3.0, -2.0)), "placed"),
        "dec_flipped": (fs, (fs[0], dec_flip), "placed"),
        "sub_box_onto_full_sky": (sub, fs, "placed"),
        "odd_output_width": (fs, odd_out, "placed"),
        "half_pixel_shift": (fs, (fs[0], _shifted(w, 0.5, 0.5)), "sprinkled"),
        "refine_2x": (fs, fine, "sprinkled"),
        "ra_flipped_quarter_shift": (fs, (fs[0], ra_flip), "sprinkled"),
        "wide_box_to_fullsky": (wide, fs500, "sprinkled"),
        "coarsen_2x": (fine, fs, "sprinkled"),
    }


CAR_CASE_NAMES = ["identity", "integer_shift", "dec_flipped", "sub_box_onto_full_sky", "odd_output_width", "half_pixel_shift",
                  "refine_2x", "ra_flipped_quarter_shift", "wide_box_to_fullsky", "coarsen_2x"]


def case_seed(name):
    """one seed per case"""
    return 100 + CAR_CASE_NAMES.index(name)


def tile_boundary_cols(xs, nx, periodic):
    """0-based source columns under the output columns either side of every multiple of 128 output columns (the tile widths
    128, 256 and 512 of the staged and LDS-DMA kernels), both taps of each"""
    out = set()
    for c in range(128, len(xs), 128):
        for oc in (c - 1, c):
            i0 = int(np.floor(xs[oc]))
            for i in (i0, i0 + 1):
                u = (i - 1) % nx if periodic else i - 1
                if 0 <= u < nx:
                    out.add(u)
    return sorted(out)


def case_map(O, kind, gin, gout, mode, seed, f32=False, nc=1, rows=()):
    """the special map of one CAR -> CAR case and its mask; placed cases add the source columns under output-tile boundaries"""
    (si, wi), (so, wo) = gin, gout
    cols = ()
    if mode == "placed":
        xs, _ = O.reproject_tables(wi, si, wo, so)
        cols = tile_boundary_cols(xs, si[0], O.is_periodic(wi, si[0]))[:24]
    return special_map(kind, si, nc=nc, seed=seed, f32=f32, mode=mode, rows=rows, cols=cols)


# ---- scattered points and the CAR <-> Gnomonic cases ---------------------------------------------------------------------------
def sky_points(rng, shape, wcs, mask, n=4000):
    """uniform on the sphere, exact pixel centres of special pixels and of their neighbours, the last half pixel beyond every
    edge, and a non-finite coordinate"""
    nx, ny = shape
    sky = np.stack([2 * np.pi * rng.random(n) - np.pi, np.arcsin(2 * rng.random(n) - 1)], axis=1)
    jj, ii = np.nonzero(mask)
    pick = rng.choice(len(jj), size=min(len(jj), 300), replace=False)
    pts = []
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            pts.append(np.stack([ii[pick] + 1.0 + di, jj[pick] + 1.0 + dj], axis=1))
    edge = rng.uniform(0.0, 0.5, 200)
    t = rng.uniform(1, nx, 200)
    u = rng.uniform(1, ny, 200)
    pts += [np.stack([1 - edge, u], axis=1), np.stack([nx + edge, u], axis=1), np.stack([t, 1 - edge], axis=1),
            np.stack([t, ny + edge], axis=1), np.stack([np.floor(t), 1 - edge], axis=1), np.stack([nx + edge, np.floor(u)], axis=1)]
    pix = np.concatenate(pts)
    a = (wcs.crval[0] + (pix[:, 0] - wcs.crpix[0]) * wcs.cdelt[0]) * wcs.unit
    d = (wcs.crval[1] + (pix[:, 1] - wcs.crpix[1]) * wcs.cdelt[1]) * wcs.unit
    sky = np.concatenate([sky, np.stack([a, d], axis=1), [[np.nan, 0.1], [0.2, np.inf]]])
    return sky


def generic_cases(pj):
    fs = pj.fullsky_geometry(2 * np.pi / 96)
    tan_small = ((64, 48), pj.Gnomonic((-2.0, 2.0), (32.5, 24.5), (175.0, 10.0)))        # straddles the RA seam of the CAR map
    tan_src = ((80, 60), pj.Gnomonic((-1.5, 1.5), (40.5, 30.5), (20.0, -15.0)))
    return {"car_to_tan": (fs, 0, tan_small, 1), "tan_to_car_half_invisible": (tan_src, 1, fs, 0)}
