"""CPU checks of the banded yardsticks and of tests/large_map_case.py: no device.

1. On the small geometries every windowed yardstick equals the corresponding rows of its dense form bit for bit, at every
   window position (every 16th and the two ends on the 1024 x 513 map, where a dense form costs 50 ms), the first and last rows
   included; a tap outside the window raises.
2. On the two large geometries each band named after a threshold straddles it, min offset < threshold <= max offset, for every
   order's taps; the last rows of a map of more than 2^31 elements lie wholly beyond 2^31.  That is what makes a device test on
   those bands sensitive to a 32-bit offset, shown without running a wrong kernel."""
import numpy as np
import pytest

import destripe_ref as DR
import large_map_case as LM
import nearest_ref as N
import normal_ref as NR
import pol_ref as P
import scatter_cubic_ref as T3
import scatter_ref as R
from conftest import bits_equal

H = 12                                        # rows of a window
GEOMS = ("cc_360x181", "box_80x40", "cc_1024x513")
N_POINTS = 3000


def _triple_equal(win, dense, rows, what):
    for a, b, name in zip(win, dense, ("ref", "k", "S")):
        b = b[..., rows, :]
        if a.dtype == np.float64:
            assert bits_equal(a, b) or (np.array_equal(np.isnan(a), np.isnan(b)) and bits_equal(np.nan_to_num(a), np.nan_to_num(b))), \
                "%s: %s differs from the dense rows" % (what, name)
        else:
            assert np.array_equal(a, b), "%s: %s differs from the dense rows" % (what, name)


class _Geom:
    """One small geometry: its points, their full-plane taps of every order, and per-point inputs."""

    def __init__(self, pj, O, geom):
        self.shape, self.wcs = R.geometries(pj)[geom]
        self.shape = (int(self.shape[0]), int(self.shape[1]))
        nx, ny = self.shape
        self.sky = N.points(O, self.wcs, self.shape, N_POINTS, 7 + len(geom))
        taps = np.concatenate([LM.order_taps(O, self.wcs, self.shape, self.sky, o) for o in (0, 1, 3)], axis=1)
        big = np.iinfo(np.int64).max
        self.row_lo = np.where(taps >= 0, taps // nx, big).min(axis=1)          # big: the point has no tap on the map
        self.row_hi = np.where(taps >= 0, taps // nx, -1).max(axis=1)
        rng = np.random.default_rng(len(geom))
        n = len(self.sky)
        self.vals = rng.normal(size=(2, n))
        self.resp = rng.normal(size=(n, 2))
        self.w = 10.0 ** rng.uniform(-1, 1, n)
        self.d = rng.normal(size=n)
        self.m3 = rng.normal(size=(3, ny, nx))
        self.out3 = rng.normal(size=(3, ny, nx))
        self.out6 = rng.normal(size=(6, ny, nx))
        self.mask = (rng.uniform(size=(ny, nx)) > 0.2) * rng.integers(1, 4, (ny, nx)).astype(float)
        self.mask.reshape(-1)[rng.integers(0, nx * ny, 5)] = np.nan

    def inside(self, row0):
        """Indices of the points whose taps all lie in rows [row0, row0 + H) or off the map."""
        return np.flatnonzero((self.row_lo >= row0) & ((self.row_hi < row0 + H) | (self.row_hi < 0)))


@pytest.fixture(scope="module", params=GEOMS)
def g(request, pj, O):
    return _Geom(pj, O, request.param)


def _positions(ny):
    step = 16 if ny > 200 else 1
    return sorted(set(range(0, ny - H + 1, step)) | {ny - H})


def test_windowed_yardsticks_equal_dense_rows(g, O):
    nx, ny = g.shape
    checked = 0
    for row0 in _positions(ny):
        at = g.inside(row0)
        if not len(at):
            continue
        checked += 1
        sky, resp, w, d, vals = g.sky[at], g.resp[at], g.w[at], g.d[at], g.vals[:, at]
        rows, win, tag = slice(row0, row0 + H), dict(row0=row0, nrows=H), "rows [%d, %d)" % (row0, row0 + H)
        a = (O, g.wcs, g.shape)
        # gathers: order 0, 1 and 3 (coefficients supplied as a band)
        assert bits_equal(N.sample(*a, g.m3[:, rows], sky, **win), N.sample(*a, g.m3, sky)), tag
        for order in (1, 3):
            got = P.sample_planes(*a, g.m3[:, rows], sky, order, order == 3, **win)
            want = P.sample_planes(*a, g.m3, sky, order, order == 3)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and bits_equal(np.nan_to_num(got), np.nan_to_num(want)), (tag, order)
        with np.errstate(invalid="ignore"):
            got, want = P.sample(*a, g.m3[:, rows], sky, resp, **win), P.sample(*a, g.m3, sky, resp)
        assert bits_equal(np.nan_to_num(got), np.nan_to_num(want)), tag
        # transposes
        t3w, t3d = T3.taps(*a, sky, **win), T3.taps(*a, sky)
        assert np.array_equal(t3w[0], np.where(t3d[0] >= 0, t3d[0] - row0 * nx, -1)) and bits_equal(t3w[1], t3d[1]), tag
        _triple_equal(T3.scatter(*a, sky, vals, out=g.out3[:2, rows], **win), T3.scatter(*a, sky, vals, out=g.out3[:2]), rows, "scatter_cubic " + tag)
        _triple_equal(T3.scatter(*a, sky, vals, **win), T3.scatter(*a, sky, vals), rows, "scatter_cubic into zeros " + tag)
        _triple_equal(R.scatter(*a, sky, vals, **win), R.scatter(*a, sky, vals), rows, "scatter " + tag)
        _triple_equal(N.scatter(*a, sky, vals, **win), N.scatter(*a, sky, vals), rows, "scatter_nearest " + tag)
        for order in (1, 3):
            for mode in (0, 1):
                out = (g.out6 if mode else g.out3)
                _triple_equal(P.scatter(*a, sky, d, resp, order, mode, out=out[:, rows], **win),
                              P.scatter(*a, sky, d, resp, order, mode, out=out), rows, "scatter_pol order %d mode %d %s" % (order, mode, tag))
        _triple_equal(N.scatter_pol(*a, sky, d, resp, 1, out=g.out6[:, rows], **win), N.scatter_pol(*a, sky, d, resp, 1, out=g.out6), rows,
                      "scatter_pol_nearest " + tag)
        # the fused passes
        _triple_equal(NR.normal(*a, g.m3[:, rows], sky, resp, w, out=g.out3[:, rows], **win), NR.normal(*a, g.m3, sky, resp, w, out=g.out3), rows,
                      "normal " + tag)
        bw, bd = N.bin(*a, sky, resp, d, w, rhs=g.out3[:, rows], weights=g.out6[:, rows], **win), N.bin(*a, sky, resp, d, w, rhs=g.out3, weights=g.out6)
        _triple_equal(bw[0], bd[0], rows, "bin rhs " + tag)
        _triple_equal(bw[1], bd[1], rows, "bin weights " + tag)
        # the destriper's passes: one detector, a chunk that starts inside a baseline
        blen, t0 = 7, 3
        nb = DR.n_base(t0 + len(at), blen)
        amp = np.random.default_rng(row0).normal(size=nb)
        lay = (1, t0, blen, nb)
        _triple_equal(DR.bin(*a, sky, resp, w, *lay, d=d, a=amp, mask=g.mask[rows], out=g.out3[:, rows], **win),
                      DR.bin(*a, sky, resp, w, *lay, d=d, a=amp, mask=g.mask, out=g.out3), rows, "baseline bin " + tag)
        pw = DR.project(*a, sky, resp, w, *lay, d=d, a=amp, m=g.m3[:, rows], mask=g.mask[rows], **win)
        pd = DR.project(*a, sky, resp, w, *lay, d=d, a=amp, m=g.m3, mask=g.mask)
        for x, y in zip(pw, pd):
            same = np.array_equal(x, y) if x.dtype != np.float64 else (np.array_equal(np.isnan(x), np.isnan(y))
                                                                      and bits_equal(np.nan_to_num(x), np.nan_to_num(y)))
            assert same, "baseline project " + tag
    assert checked >= 0.9 * len(_positions(ny))


def test_a_tap_outside_the_window_raises(g, O):
    nx, ny = g.shape
    row0 = ny // 2
    a = (O, g.wcs, g.shape)
    win = dict(row0=row0, nrows=H)
    near = np.flatnonzero((g.row_lo == row0 - 1) & (g.row_hi >= row0))[:3]        # straddle the window's lower edge
    assert len(near)
    at = np.concatenate([g.inside(row0)[:50], near])
    sky, resp, w, d = g.sky[at], g.resp[at], g.w[at], g.d[at]
    rows = slice(row0, row0 + H)
    calls = [lambda: T3.taps(*a, sky, **win), lambda: T3.scatter(*a, sky, d, **win),
             lambda: P.sample_planes(*a, g.m3[:, rows], sky, 3, True, **win)]
    for call in calls:
        with pytest.raises(ValueError, match="outside the resident rows"):
            call()
    # order 1: a point whose cell has its lower row before the window and its upper row in it
    t1 = LM.order_taps(O, g.wcs, g.shape, g.sky, 1)
    near = np.flatnonzero((t1[:, 0] >= 0) & (t1[:, 0] // nx == row0 - 1) & (t1[:, 2] // nx == row0))[:3]
    assert len(near)
    at = np.concatenate([g.inside(row0)[:50], near])
    sky, resp, w = g.sky[at], g.resp[at], g.w[at]
    with pytest.raises(ValueError, match="outside the resident rows"):
        NR.normal(*a, g.m3[:, rows], sky, resp, w, **win)
    # order 0: a point whose own pixel lies on the row before the window
    cells = N.taps(*a, g.sky)[0]
    out0 = np.flatnonzero((cells >= 0) & (cells // nx == row0 - 1))[:2]
    assert len(out0)
    at = np.concatenate([g.inside(row0)[:50], out0])
    sky, resp, w, d = g.sky[at], g.resp[at], g.w[at], g.d[at]
    calls = [lambda: N.bin(*a, sky, resp, d, w, **win),
             lambda: DR.bin(*a, sky, resp, w, 1, 0, 7, DR.n_base(len(at), 7), d=d, **win),
             lambda: DR.project(*a, sky, resp, w, 1, 0, 7, DR.n_base(len(at), 7), d=d, m=g.m3[:, rows], **win)]
    for call in calls:
        with pytest.raises(ValueError, match="outside the resident rows"):
            call()


# ---- the two large geometries ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tier,nc", [("R", 1), ("R", 3), ("P", 3), ("P", 6)])
def test_threshold_bands_straddle_their_threshold(pj, O, tier, nc):
    shape, wcs = (LM.tier_r if tier == "R" else LM.tier_p)(pj)
    case = LM.Case(O, shape, wcs, nc)
    nx, ny = shape
    plane = nx * ny
    names = [b.name for b in case.bands]
    print("tier %s, %d planes of %d x %d: %r, %d points" % (tier, nc, nx, ny, case.bands, case.n_points()))
    assert names[0] == "first" and names[-1] == "last" and case.bands[0].rows == slice(0, 8) and case.bands[-1].rows == slice(ny - 8, ny)
    assert names[1:-1] == [name for name, t in LM.THRESHOLDS if t < nc * plane]
    assert 2000 <= case.n_points() <= 6000
    for b, band in enumerate(case.bands):
        if band.threshold is None:
            continue
        assert band.nrows >= 16 and band.row0 <= band.cross[0] < band.row0 + band.nrows
        assert band.plane * plane + band.cross[0] * nx + band.cross[1] == band.threshold
        for order in (0, 1, 3):
            lo, hi = case.offsets(O, b, band.plane, order)
            assert lo < band.threshold <= hi, (band, order, lo, hi)
    if nc * plane > 2 ** 31:
        for order in (0, 1, 3):
            lo, hi = case.offsets(O, len(case.bands) - 1, nc - 1, order)
            assert lo > 2 ** 31 and hi < nc * plane, (order, lo, hi)
    # what the issue says of the two geometries, from the shapes
    if tier == "R":
        assert plane > 2 ** 31 and (2 ** 31) // nx == 24855                    # jr * nx alone passes 2^31 from row 24856 (1-based) on
        if nc == 3:
            assert plane > 2 ** 31 and 2 * plane > 2 ** 32 and names == ["first", "2^29", "2^31", "2^32", "last"]
    else:
        assert plane % 2 == 0
        if nc == 3:
            assert 2 * plane < 2 ** 31 < 3 * plane
        else:
            assert 4 * plane < 2 ** 32 < 5 * plane
