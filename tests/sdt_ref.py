"""Brute-force yardstick for distance_transform, transform_distance.jl:55-78 step for step in numpy: the pixel centres'
RA / DEC as :56-57 take them (pix2sky over 1:nx and 1:ny with the per-element rewind: the oracle's PXL_WRAP_REWIND), the
list of zero pixels (:59-64, iszero), for every pixel the squared chord to every zero in `metric`'s difference form
(:81-92), the minimum, acos(1 - d2/2).  The sampled form takes a list of pixels and an explicit list of zeros, for maps too
large for the full table.  Also the per-pixel error bound the device is held to, seeded masks, and `emulate`:
the device's two kernels (csrc/pxl_distance.h) transliterated to numpy, with four named one-line mutations.  The emulation is
not a yardstick.  tests/test_sdt_ref.py runs it, whole and mutated, on the masks of the device tests to show that those masks
tell a right kernel from a subtly wrong one."""
import math

import numpy as np

from oracle import oracle as O

EPS = 2.0 ** -52


def sky_angles(wcs, shape):
    """(alphas, deltas) of transform_distance.jl:56-57."""
    nx, ny = int(shape[0]), int(shape[1])
    ra = O.pix2sky(wcs, np.column_stack([np.arange(1, nx + 1, dtype=float), np.ones(nx)]), O.WRAP_REWIND)[:, 0]
    dec = O.pix2sky(wcs, np.column_stack([np.ones(ny), np.arange(1, ny + 1, dtype=float)]), O.WRAP_REWIND)[:, 1]
    return ra, dec


def _tables(wcs, shape):
    ra, dec = sky_angles(wcs, shape)
    return np.cos(ra), np.sin(ra), np.cos(dec), np.sin(dec)


def _d2(t, i1, j1, i2, j2):
    """metric(): x = cos(d) cos(a), y = cos(d) sin(a), z = sin(d); (x1 - x2)^2 + (y1 - y2)^2 + (z1 - z2)^2, left to right."""
    ca, sa, cd, sd = t
    x1, y1, z1 = cd[j1] * ca[i1], cd[j1] * sa[i1], sd[j1]
    x2, y2, z2 = cd[j2] * ca[i2], cd[j2] * sa[i2], sd[j2]
    return (x1 - x2) ** 2 + (y1 - y2) ** 2 + (z1 - z2) ** 2


def sampled(wcs, shape, ii, jj, zi, zj, cap=None, chunk=256):
    """Distances of the pixels (ii, jj) (0-based column, row) to the nearest of the zeros (zi, zj).  cap: optional per-pixel
    upper bound on that distance; then only zeros whose DEC lies within it of the pixel's are scanned (|DEC difference| never
    exceeds the angular distance), which leaves the minimum unchanged.  inf where no zero is listed."""
    t = _tables(wcs, shape)
    _, dec = sky_angles(wcs, shape)
    ii, jj = np.asarray(ii, dtype=np.int64), np.asarray(jj, dtype=np.int64)
    zi, zj = np.asarray(zi, dtype=np.int64), np.asarray(zj, dtype=np.int64)
    out = np.full(ii.size, np.inf)
    if zi.size == 0:
        return out
    if cap is None:
        for s in range(0, ii.size, chunk):
            d2 = _d2(t, ii[s:s + chunk, None], jj[s:s + chunk, None], zi[None, :], zj[None, :])
            out[s:s + chunk] = np.arccos(1 - d2.min(axis=1) / 2)
        return out
    ra, _ = sky_angles(wcs, shape)
    order = np.argsort(dec[zj], kind="stable")
    zi, zj = zi[order], zj[order]
    zdec, zra = dec[zj], ra[zi]
    for k in range(ii.size):
        rho, dk = cap[k] + 1e-9, dec[jj[k]]
        lo, hi = np.searchsorted(zdec, [dk - rho, dk + rho], side="left")
        if hi <= lo:
            continue
        ci, cj = zi[lo:hi], zj[lo:hi]
        if abs(dk) + rho < math.pi / 2 - 1e-6:     # a cap that misses both poles spans asin(sin rho / cos dec) either way in RA
            h = math.asin(min(1.0, math.sin(rho) / math.cos(dk))) + 1e-9
            near = np.abs(np.remainder(zra[lo:hi] - ra[ii[k]] + math.pi, 2 * math.pi) - math.pi) <= h
            ci, cj = ci[near], cj[near]
        d2 = _d2(t, ii[k], jj[k], ci, cj)
        out[k] = np.arccos(np.array([1 - d2.min() / 2]))[0]
    return out


def distance_transform(m, wcs):
    """m: (ny, nx) host array.  The reference's BruteForceSDT result (ny, nx), or None where it raises (no zero pixel)."""
    ny, nx = m.shape
    zj, zi = np.nonzero(m == 0)
    if zi.size == 0:
        return None
    jj, ii = np.divmod(np.arange(nx * ny), nx)
    return sampled(wcs, (nx, ny), ii, jj, zi, zj).reshape(ny, nx)


def bound(theta):
    """Per-pixel bound on |theta_device - theta_ref|.  In the chord d = 2 sin(theta/2):
    (i) the device's cos / sin tables against the host's: within 1 ulp each, so <= 4 eps d in d^2;
    (ii) the choice of the zero in the dot-product form: <= 4 eps absolute in d^2 (a near-tie may pick the other zero);
    (iii) the rounding of 1 - d^2/2 before acos, 1.1e-16 on each side; acos itself, 1 ulp on each side.
    theta moves by 1 / sin(theta) per unit of 1 - d^2/2, so the bound is (2 eps (1 + d) + 2.2e-16) / sin(theta) + 2 ulp;
    it is never looser than the ceiling 4e-15 / max(sin theta, 1e-3) + 8 ulp(theta)."""
    theta = np.asarray(theta, dtype=float)
    s = np.sin(theta)
    d = 2 * np.sin(theta / 2)
    with np.errstate(divide="ignore"):
        derived = (2 * EPS * (1 + d) + 2.2e-16) / s + 2 * np.spacing(theta)
    ceiling = 4e-15 / np.maximum(s, 1e-3) + 8 * np.spacing(theta)
    return np.minimum(np.where(s > 0, derived, np.inf), ceiling)


def worst_ratio(got, ref):
    """max |got - ref| / bound(ref) over the pixels (0 if all agree)."""
    err = np.abs(np.asarray(got, dtype=float) - np.asarray(ref, dtype=float))
    return float((err / bound(ref)).max()) if err.size else 0.0


def disk_zeros(wcs, shape, ncent, radius, seed):
    """(zi, zj) of a point-source mask: every pixel whose centre lies within `radius` of one of `ncent` seeded centres drawn
    uniformly on the sphere (only the rows within `radius` of a centre are scanned)."""
    nx, ny = int(shape[0]), int(shape[1])
    ca, sa, cd, sd = _tables(wcs, shape)
    _, dec = sky_angles(wcs, shape)
    rng = np.random.default_rng(seed)
    zc = rng.uniform(-1.0, 1.0, ncent)
    ac = rng.uniform(-math.pi, math.pi, ncent)
    dc = np.arcsin(zc)
    ra, _ = sky_angles(wcs, shape)
    out_i, out_j = [], []
    cr = math.cos(radius)
    for k in range(ncent):
        rows = np.nonzero(np.abs(dec - dc[k]) <= radius + 1e-12)[0]
        if rows.size == 0:
            continue
        cols = np.arange(nx)
        if abs(dc[k]) + radius < math.pi / 2 - 1e-6:       # the cap misses both poles: its RA half-width is asin(sin r / cos d)
            h = math.asin(min(1.0, math.sin(radius) / math.cos(dc[k]))) + 1e-9
            cols = np.nonzero(np.abs(np.remainder(ra - ac[k] + math.pi, 2 * math.pi) - math.pi) <= h)[0]
        cosang = (sd[rows, None] * math.sin(dc[k])
                  + cd[rows, None] * math.cos(dc[k]) * (ca[None, cols] * math.cos(ac[k]) + sa[None, cols] * math.sin(ac[k])))
        r, c = np.nonzero(cosang >= cr)
        out_j.append(rows[r])
        out_i.append(cols[c])
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    z = np.unique(np.concatenate(out_j) * nx + np.concatenate(out_i))
    return z % nx, z // nx


def band_rows(wcs, shape, halfwidth):
    """Rows of the band |DEC| < halfwidth."""
    _, dec = sky_angles(wcs, shape)
    return np.nonzero(np.abs(dec) < halfwidth)[0]


# ---- the device's method in numpy -------------------------------------------------------------------------------------

MUTATIONS = ("no_wrap", "own_word", "sweep_inverted", "no_pops")


def _emulate_rows(m, ca, sa, mutate):
    """k_sdt_rows: best[j, i] = column of row j's best zero for column i, -1 where the row has none.  The candidates are
    the nearest zero at or left of i and at or right of it, each wrapping to the row's last / first zero, and the choice is
    `cr > cl ? r : l` on the table dot products.  no_wrap: a missing candidate is replaced by the other one, not by the
    zero round the seam or gap.  own_word: the left candidate comes from the 64-column words before the pixel's own."""
    ny, nx = m.shape
    cols = np.arange(nx)
    best = np.full((ny, nx), -1, np.int64)
    for j in range(ny):
        z = np.nonzero(m[j] == 0)[0]
        if z.size == 0:
            continue
        kl = np.searchsorted(z, (cols >> 6) * 64 - 1 if mutate == "own_word" else cols, side="right") - 1
        kr = np.searchsorted(z, cols, side="left")
        hasl, hasr = kl >= 0, kr < z.size
        l, r = z[np.maximum(kl, 0)], z[np.minimum(kr, z.size - 1)]
        if mutate == "no_wrap":
            l = np.where(hasl, l, r)
            r = np.where(hasr, r, l)
        else:
            l = np.where(hasl, l, z[-1])
            r = np.where(hasr, r, z[0])
        cl = ca * ca[l] + sa * sa[l]
        cr = ca * ca[r] + sa * sa[r]
        best[j] = np.where(l == r, l, np.where(cr > cl, r, l))
    return best


def emulate(m, wcs, mutate=None):
    """m: (ny, nx) host array.  k_sdt_rows and k_sdt_columns of csrc/pxl_distance.h step for step, all columns at once, with
    the cos / sin tables taken from numpy: the same products and comparisons in the same order (no fused multiply-add).
    Per column the chain over the rows that have a zero, in order of increasing DEC, with the `<= 0` pop rule and the
    re-read of the second vertex after a pop; the query sweep in the same order with a pointer that only moves forward on
    `>=`; points use fmax(cos d, 0); zero pixels are 0; the chosen zero's distance in the difference form.
    mutate: None, or one of MUTATIONS.  sweep_inverted: both sweeps run against DEC.  no_pops: the chain keeps every point.
    Returns (ny, nx); +inf everywhere if m has no zero."""
    assert mutate is None or mutate in MUTATIONS, mutate
    ny, nx = m.shape
    ca, sa, cd, sd = _tables(wcs, (nx, ny))
    up = wcs.cdelt[1] * wcs.unit > 0.0
    if mutate == "sweep_inverted":
        up = not up
    best = _emulate_rows(m, ca, sa, mutate)
    cols = np.arange(nx)
    cdp = np.fmax(cd, 0.0)
    order = range(ny) if up else range(ny - 1, -1, -1)

    def point(i, rows, c):
        return cdp[rows] * (ca[i] * ca[c] + sa[i] * sa[c]), sd[rows]

    chr_, chc = np.zeros((nx, ny), np.int64), np.zeros((nx, ny), np.int64)
    n = np.zeros(nx, np.int64)
    x0, y0, x1, y1 = np.zeros(nx), np.zeros(nx), np.zeros(nx), np.zeros(nx)
    for j in order:
        c = best[j]
        act = c >= 0
        if not act.any():
            continue
        px, py = point(cols, j, np.where(act, c, 0))
        py = np.full(nx, py)
        while mutate != "no_pops":
            pop = act & (n >= 2) & ((x0 - x1) * (py - y1) - (y0 - y1) * (px - x1) <= 0.0)
            if not pop.any():
                break
            n[pop] -= 1
            x0[pop], y0[pop] = x1[pop], y1[pop]
            i = np.nonzero(pop & (n >= 2))[0]
            x1[i], y1[i] = point(i, chr_[i, n[i] - 2], chc[i, n[i] - 2])
        i = np.nonzero(act)[0]
        chr_[i, n[i]], chc[i, n[i]] = j, c[i]
        n[i] += 1
        x1[i], y1[i], x0[i], y0[i] = x0[i], y0[i], px[i], py[i]
    if not n.any():
        return np.full((ny, nx), np.inf)
    assert n.all()                       # a row with a zero gives every column a point
    out = np.empty((ny, nx))
    k = np.zeros(nx, np.int64)
    xk, yk = point(cols, chr_[cols, 0], chc[cols, 0])
    xn, yn = np.zeros(nx), np.zeros(nx)
    i = np.nonzero(n > 1)[0]
    xn[i], yn[i] = point(i, chr_[i, 1], chc[i, 1])
    for j in order:
        ux, uy = cd[j], sd[j]
        while True:
            adv = (k + 1 < n) & (ux * xn + uy * yn >= ux * xk + uy * yk)
            if not adv.any():
                break
            k[adv] += 1
            xk[adv], yk[adv] = xn[adv], yn[adv]
            i = np.nonzero(adv & (k + 1 < n))[0]
            xn[i], yn[i] = point(i, chr_[i, k[i] + 1], chc[i, k[i] + 1])
        zr, zc = chr_[cols, k], chc[cols, k]
        xa, ya, za = ux * ca, ux * sa, uy
        xb, yb, zb = cd[zr] * ca[zc], cd[zr] * sa[zc], sd[zr]
        d2 = (xa - xb) * (xa - xb) + (ya - yb) * (ya - yb) + (za - zb) * (za - zb)
        out[j] = np.where(best[j] == cols, 0.0, np.arccos(1.0 - d2 / 2.0))
    return out


# ---- masks and geometries shared by tests/test_sdt_ref.py and tests/test_gpu_distance_transform.py ---------------------

DENSE_MASKS = ("ellipse", "ellipse_complement", "half_plane", "checkerboard", "random50", "random90", "random99",
               "alternate_rows", "full_column", "staircase", "crossing_staircases")
DENSE_GEOMETRIES = ("cc4", "cc3", "fejer4", "box1", "gap4_dec_down")


def dense_geometry(pj, name):
    """(shape, wcs): 4 and 3 degree full-sky CC (90 x 46, 120 x 61), 4 degree full-sky Fejer1 (90 x 45, rows half a pixel
    off the poles), a 40 x 20 box at 1 degree, a 300-degree box at 4 degrees with DEC running downwards (75 x 15).
    The row counts leave 2, 1, 1, 0 and 3 modulo the column kernel's batch of 4."""
    deg = math.pi / 180
    if name == "cc4":
        return pj.fullsky_geometry(4 * deg)
    if name == "cc3":
        return pj.fullsky_geometry(3 * deg)
    if name == "fejer4":
        return (90, 45), pj.CarFejer1((-4.0, 4.0), (45.5, 23.0), (2.0, 0.0))
    if name == "box1":
        return pj.geometry([[20 * deg, -20 * deg], [-10 * deg, 10 * deg]], 1 * deg)
    if name == "gap4_dec_down":
        return pj.geometry([[150 * deg, -150 * deg], [30 * deg, -30 * deg]], 4 * deg)
    raise KeyError(name)


def dense_mask(name, nx, ny):
    """(ny, nx) of ones with zeros in large connected or dense regions (seeded where random).  ellipse: a footprint, zero
    outside an ellipse about the map's centre; ellipse_complement: zero inside it; half_plane: zero below a diagonal;
    checkerboard; random50 / 90 / 99: that percentage of zeros; alternate_rows: every even row; full_column: one column;
    staircase: one zero per column on a rising diagonal (a run of zeros per row, every row a chain point);
    crossing_staircases: that and the falling diagonal."""
    jj, ii = np.mgrid[0:ny, 0:nx]
    m = np.ones((ny, nx))
    inside = ((ii - (nx - 1) / 2) / (0.35 * nx)) ** 2 + ((jj - (ny - 1) / 2) / (0.3 * ny)) ** 2 <= 1.0
    if name == "ellipse":
        m[~inside] = 0.0
    elif name == "ellipse_complement":
        m[inside] = 0.0
    elif name == "half_plane":
        m[ii * ny + jj * nx < nx * ny] = 0.0
    elif name == "checkerboard":
        m[(ii + jj) % 2 == 0] = 0.0
    elif name.startswith("random"):
        pct = int(name[6:])
        m[np.random.default_rng(1000 * pct + nx).random((ny, nx)) < pct / 100] = 0.0
    elif name == "alternate_rows":
        m[0::2] = 0.0
    elif name == "full_column":
        m[:, nx // 3] = 0.0
    elif name == "staircase":
        m[(ii * ny) // nx == jj] = 0.0
    elif name == "crossing_staircases":
        m[((ii * ny) // nx == jj) | (((nx - 1 - ii) * ny) // nx == jj)] = 0.0
    else:
        raise KeyError(name)
    return m


WORD_EDGE_NX = (63, 64, 65, 128, 129, 200)
WORD_EDGE_ROWS = ("col0", "last_col", "both_ends", "z63_64", "z127_128_129", "inside_one_word", "last_word_only", "all", "none",
                  "random_half")


def word_edge_geometry(pj, nx, dec_down=False, ra_up=False):
    """An nx x 10 box of 0.02 degree columns and 5 degree rows: a row spans at most 4 degrees, less than the distance to
    the next row, so the zeros of a pixel's own row decide it (where the row has any)."""
    deg = math.pi / 180
    ra = nx * 0.01 * (-1 if ra_up else 1)
    dec = 25.0 * (-1 if dec_down else 1)
    return pj.geometry([[ra * deg, -ra * deg], [-dec * deg, dec * deg]], (0.02 * deg, 5 * deg))


def word_edge_mask(nx):
    """(10, nx): one row per pattern of WORD_EDGE_ROWS, around the 64-column words of the device's row mask.  Columns a
    pattern names beyond nx - 1 are left out (a row left with none is a second row without a zero)."""
    m = np.ones((len(WORD_EDGE_ROWS), nx))
    last_word = ((nx - 1) >> 6) * 64
    pats = {"col0": [0], "last_col": [nx - 1], "both_ends": [0, nx - 1], "z63_64": [63, 64], "z127_128_129": [127, 128, 129],
            "inside_one_word": [3, 17, 18, 40, 62, 69, 97, 126], "last_word_only": [(last_word + nx - 1) // 2],
            "all": list(range(nx)), "none": [],
            "random_half": list(np.nonzero(np.random.default_rng(nx).random(nx) < 0.5)[0])}
    for j, name in enumerate(WORD_EDGE_ROWS):
        z = [c for c in pats[name] if c < nx]
        m[j, z] = 0.0
    return m


SCAN_TRIP_CASES = ("z65535_65536", "every_256", "words_1024_up", "z65535", "z65536", "z4479", "z4480")


def scan_trip_mask(case, nx=70000, ny=3):
    """70000 columns are 1094 mask words: the prefix scan of the words' last zeros runs over words 0..1023, then 1024..1093
    with a carry, and the suffix scan of their first zeros over words 1093..70, then 69..0.  One row carries zeros and the
    other two have none, so that row decides every pixel.  z65535_65536: the last bit of word 1023 and the first of word
    1024; every_256: a zero in every fourth word; words_1024_up: zeros in the second prefix trip only; z65535 / z65536: one
    of the two alone, so every word on the far side of the prefix carry (and the row's last zero) depends on it; z4479 /
    z4480: the last bit of word 69 and the first of word 70 alone, the same for the suffix carry."""
    m = np.ones((ny, nx))
    z = {"z65535_65536": [65535, 65536], "every_256": list(range(0, nx, 256)), "words_1024_up": [65600, 66000, 67500, 69999],
         "z65535": [65535], "z65536": [65536], "z4479": [4479], "z4480": [4480]}[case]
    m[SCAN_TRIP_CASES.index(case) % ny, z] = 0.0
    return m


FAR_CASES = ("off_pole", "pole_row", "antipodal_pair", "antipodal_rows")


def far_mask(case, nx, ny):
    """A single zero off the poles, a single zero on a pole row, two zeros half the sky apart in one row: most pixels lie
    on the far hemisphere of the nearest zero, where the chain's points have negative x.  antipodal_rows: three zeros in
    three rows, half and a quarter of the sky apart in RA, so a column's chain mixes points of negative and positive x."""
    m = np.ones((ny, nx))
    if case == "antipodal_rows":
        assert nx % 2 == 0
        m[[ny // 4, ny // 2, (3 * ny) // 4], [nx // 9, nx // 9 + nx // 2, nx // 9 + nx // 4]] = 0.0
        return m
    if case == "off_pole":
        m[(2 * ny) // 3, nx // 9] = 0.0
    elif case == "pole_row":
        m[ny - 1, nx // 9] = 0.0
    elif case == "antipodal_pair":
        assert nx % 2 == 0
        m[ny // 3, [nx // 9, nx // 9 + nx // 2]] = 0.0
    else:
        raise KeyError(case)
    return m


REFUSED = ("131073 columns", "top row beyond DEC 90", "361 columns of 1 degree", "row step of 354 degrees")


def refused_geometry(pj, what):
    """(shape, wcs, the reason the entry's message must give) of a geometry pxl_distance_transform_car_f64 refuses.  Each
    passes every check before its own.  A row step of nearly a whole turn, which rewind folds back, is the only way past
    the pole check with DEC not monotone."""
    deg = math.pi / 180
    if what == "131073 columns":
        return (131073, 1), pj.CarClenshawCurtis((-0.001, 0.001), (65537.0, 1.0), (0.0, 0.0)), "more than 131072 pixels"
    if what == "top row beyond DEC 90":            # 22 rows of 0.5 degrees from DEC 80: the last lies at 90.5 degrees
        shape, wcs = pj.geometry([[20 * deg, -20 * deg], [80 * deg, 91 * deg]], 0.5 * deg)
        assert shape == (80, 22)
        return shape, wcs, "row 22 lies beyond a pole"
    if what == "361 columns of 1 degree":
        return (361, 2), pj.CarClenshawCurtis((-1.0, 1.0), (181.0, 1.0), (0.0, 0.0)), "more than 360 degrees of RA"
    if what == "row step of 354 degrees":
        return (8, 2), pj.CarClenshawCurtis((-1.0, 354.0), (1.0, 1.0), (0.0, 3.0)), "DEC is not monotone"
    raise KeyError(what)


DENSE_CASES = tuple("dense/%s/%s" % (g, k) for g in DENSE_GEOMETRIES for k in DENSE_MASKS)
WORD_EDGE_CASES = tuple("word_edge/%d" % nx for nx in WORD_EDGE_NX)          # 129: DEC downwards, 200: RA increasing
ALL_CASES = (DENSE_CASES + WORD_EDGE_CASES + tuple("far/" + c for c in FAR_CASES)
             + tuple("scan/" + c for c in SCAN_TRIP_CASES))
_CASES = {}


def case(pj, name):
    """name of ALL_CASES -> (m, shape, wcs, ref): the mask (ny, nx), its geometry and the brute-force distances, built once
    and shared (read-only) by every test that names the case."""
    if name not in _CASES:
        deg = math.pi / 180
        kind, _, rest = name.partition("/")
        if kind == "dense":
            g, _, k = rest.partition("/")
            shape, wcs = dense_geometry(pj, g)
            m = dense_mask(k, *shape)
        elif kind == "word_edge":
            nx = int(rest)
            shape, wcs = word_edge_geometry(pj, nx, dec_down=nx == 129, ra_up=nx == 200)
            assert shape == (nx, len(WORD_EDGE_ROWS)) and (wcs.cdelt[1] < 0) == (nx == 129) and (wcs.cdelt[0] > 0) == (nx == 200)
            m = word_edge_mask(nx)
        elif kind == "far":
            shape, wcs = pj.fullsky_geometry(4 * deg)
            m = far_mask(rest, *shape)
        elif kind == "scan":
            shape, wcs = pj.geometry([[175 * deg, -175 * deg], [0.0, 0.015 * deg]], 0.005 * deg)
            assert shape == (70000, 3)
            m = scan_trip_mask(rest, *shape)
        else:
            raise KeyError(name)
        ref = distance_transform(m, wcs)
        m.setflags(write=False)
        ref.setflags(write=False)
        _CASES[name] = (m, shape, wcs, ref)
    return _CASES[name]
