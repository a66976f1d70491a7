"""distance_transform on the device (pxl_distance_transform_car_f64 through pj.distance_transform) against the brute-force
yardstick tests/sdt_ref.py.  Every pixel is held to the per-pixel bound sdt_ref.bound (derived, not fitted);
zero pixels must be exactly 0.0.  Each check prints its worst ratio of error to bound."""
import ctypes as C
import math

import numpy as np
import pytest

import sdt_ref as R
from conftest import ARCMIN, DEG, bits_equal

torch = pytest.importorskip("torch")
from gpu_support import dev
pytestmark = pytest.mark.gpu


def _box(pj, ra1, ra2, dec1, dec2, res):
    return pj.geometry([[ra1 * DEG, ra2 * DEG], [dec1 * DEG, dec2 * DEG]], res * DEG)


def _device(pj, dev, m, wcs, dt=None):
    em = pj.Enmap(torch.from_numpy(np.ascontiguousarray(m)).to(dev), wcs)
    return pj.distance_transform(dt if dt is not None else pj.ExactSeqSDT(), em).data.cpu().numpy()


def _check(got, m, wcs, what, ref=None):
    if ref is None:
        ref = R.distance_transform(m, wcs)
    zero = m == 0
    assert np.array_equal(got[zero].view(np.int64), np.zeros(int(zero.sum()), np.int64)), what     # exactly +0.0
    r = R.worst_ratio(got, ref)
    print("%s: worst error / bound = %.3g" % (what, r))
    assert r <= 1.0, what
    return r


def test_reference_testset_different_implementations(pj, dev):
    """test_distance_transform.jl:2-23: the 0.5 degree box [20 -20; -10 10] (80 x 40), 300 seeded masks of 30 interior
    zeros, all three kinds against the brute-force yardstick, every pixel within the bound."""
    shape, wcs = _box(pj, 20, -20, -10, 10, 0.5)
    nx, ny = shape
    assert shape == (80, 40)
    rng = np.random.default_rng(2024)
    worst = 0.0
    for kk in range(300):
        m = np.ones((ny, nx))
        m[rng.integers(1, ny - 1, 30), rng.integers(1, nx - 1, 30)] = 0.0       # rand(2:size-1), 1-based
        outs = [_device(pj, dev, m, wcs, dt) for dt in (pj.ExactSeqSDT(), pj.BruteForceSDT(), pj.ApproxSeqSDT())]
        assert bits_equal(outs[0], outs[1]) and bits_equal(outs[0], outs[2])
        worst = max(worst, _check(outs[0], m, wcs, "box mask %d" % kk))
    print("300 masks: worst error / bound = %.3g" % worst)


def test_reference_testset_metric(pj, dev):
    """test_distance_transform.jl:26-44 on the device: m[1,1] = 0 on the box [20 -20; 0 10]."""
    shape, wcs = _box(pj, 20, -20, 0, 10, 0.5)
    nx, ny = shape
    m = np.ones((ny, nx))
    m[0, 0] = 0.0
    dist = _device(pj, dev, m, wcs)
    ra, dec = R.sky_angles(wcs, shape)
    rtol = np.sqrt(np.finfo(float).eps)
    for i in range(nx):
        a, b = ra[0] - ra[i], dist[0, i]
        assert abs(a - b) <= rtol * max(abs(a), abs(b)), i
    for j in range(ny):
        a, b = dec[j] - dec[0], dist[j, 0]
        assert abs(a - b) <= rtol * max(abs(a), abs(b)), j
    _check(dist, m, wcs, "metric testset")


@pytest.mark.parametrize("res", [1.0, 4.0])
@pytest.mark.parametrize("kind", ["seam", "poles", "random"])
def test_full_sky(pj, dev, res, kind):
    """Full-sky CC maps: zeros on both seam columns (the nearest zero lies across RA = +-180), on the pole rows, at random."""
    shape, wcs = pj.fullsky_geometry(res * DEG)
    nx, ny = shape
    rng = np.random.default_rng(int(res * 10) + len(kind))
    m = np.ones((ny, nx))
    if kind == "seam":
        rows = rng.integers(0, ny, 6)
        m[rows[:3], 0] = 0.0
        m[rows[3:], nx - 1] = 0.0
    elif kind == "poles":
        m[0, rng.integers(0, nx, 3)] = 0.0
        m[ny - 1, rng.integers(0, nx, 3)] = 0.0
        m[rng.integers(1, ny - 1, 4), rng.integers(0, nx, 4)] = 0.0
    else:
        m[rng.integers(0, ny, 40), rng.integers(0, nx, 40)] = 0.0
    _check(_device(pj, dev, m, wcs), m, wcs, "full sky %g deg, %s" % (res, kind))


@pytest.mark.parametrize("case", ["wide_gap", "dec_down", "ra_up", "one_row", "one_column", "odd_nx"])
def test_geometries(pj, dev, case):
    """A 300-degree box (the nearest zero of a row can lie round the gap), cdelt[2] < 0, cdelt[1] > 0, a single row, a
    single column, nx not a multiple of 64."""
    boxes = {"wide_gap": (150, -150, -30, 30, 1.0), "dec_down": (20, -20, 10, -10, 0.5), "ra_up": (-20, 20, -10, 10, 0.5),
             "one_row": (40, -40, 0, 0.5, 0.5), "one_column": (0.5, 0, -30, 30, 0.5), "odd_nx": (50.5, -50, -20, 20, 0.5)}
    shape, wcs = _box(pj, *boxes[case])
    nx, ny = shape
    if case == "one_row":
        assert ny == 1
    if case == "one_column":
        assert nx == 1
    if case == "odd_nx":
        assert nx % 64 != 0
    rng = np.random.default_rng(len(case))
    m = np.ones((ny, nx))
    if case == "wide_gap":
        m[rng.integers(0, ny, 4), rng.integers(0, 5, 4)] = 0.0          # zeros near the left edge only: pixels near the right
        m[rng.integers(0, ny, 2), nx - 1] = 0.0                          # edge reach them round the 60-degree gap
    else:
        nz = max(1, (nx * ny) // 400)
        m[rng.integers(0, ny, nz), rng.integers(0, nx, nz)] = 0.0
    _check(_device(pj, dev, m, wcs), m, wcs, case)


def test_special_masks(pj, dev):
    """All zeros -> exactly 0 everywhere; a single zero; -0.0 counts and NaN does not; no zero -> ValueError in Python and
    +Inf everywhere from the C entry."""
    shape, wcs = _box(pj, 20, -20, -10, 10, 0.5)
    nx, ny = shape
    got = _device(pj, dev, np.zeros((ny, nx)), wcs)
    assert np.array_equal(got.view(np.int64), np.zeros((ny, nx), np.int64))
    m = np.ones((ny, nx))
    m[17, 33] = 0.0
    one = _device(pj, dev, m, wcs)
    _check(one, m, wcs, "single zero")
    m2 = np.ones((ny, nx))
    m2[17, 33] = -0.0
    m2[5, 5] = np.nan
    m2[30, 70] = np.nan
    assert bits_equal(_device(pj, dev, m2, wcs), one)
    none = np.ones((ny, nx))
    none[3, 3] = np.nan
    with pytest.raises(ValueError, match="no zero"):
        _device(pj, dev, none, wcs)
    src = torch.from_numpy(none).to(dev)
    dst = torch.zeros_like(src)
    lib = pj.load_library()
    rc = lib.pxl_distance_transform_car_f64(C.byref(wcs.to_struct()), pj._lib.shape_arr(shape), C.c_void_p(src.data_ptr()),
                                            C.c_void_p(dst.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, pj._lib.last_error()
    torch.cuda.synchronize()
    assert torch.isinf(dst).all() and (dst > 0).all()


def _sampled_check(pj, dev, shape, wcs, m_dev, zi, zj, what, nsamp=8192):
    """8192 seeded pixels of the device result against the sampled yardstick; zero pixels exactly 0."""
    nx, ny = shape
    out = pj.distance_transform(pj.ExactSeqSDT(), pj.Enmap(m_dev, wcs)).data
    rng = np.random.default_rng(nx)
    ii, jj = rng.integers(0, nx, nsamp), rng.integers(0, ny, nsamp)
    idx = torch.from_numpy(jj * nx + ii).to(dev)
    got = out.view(-1)[idx].cpu().numpy()
    isz = (m_dev.view(-1)[idx] == 0).cpu().numpy()
    assert np.array_equal(got[isz].view(np.int64), np.zeros(int(isz.sum()), np.int64)), what
    keep = ~isz
    ref = R.sampled(wcs, shape, ii[keep], jj[keep], zi, zj, cap=got[keep])
    r = R.worst_ratio(got[keep], ref)
    print("%s: %d pixels (%d zero), worst error / bound = %.3g" % (what, nsamp, int(isz.sum()), r))
    assert r <= 1.0, what
    del out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("geom", ["4099x2113", "43200x21601"])
@pytest.mark.parametrize("mask", ["sources", "band"])
def test_large_maps_sampled(pj, dev, geom, mask):
    """4099 x 2113 and 43200 x 21601 CC maps with a point-source mask (2000 disks, 5 arcmin or 3 pixels) and a band
    |DEC| < 10 degrees.  The band's explicit zero list is its two edge rows: every zero row of a band is complete, so for a
    pixel outside it the nearest zero of a row is in the pixel's own column, and the nearest of those is in the edge row on
    its side."""
    if geom == "4099x2113":
        shape, wcs = pj.fullsky_geometry((2 * math.pi / 4099, math.pi / 2112))
    else:
        shape, wcs = pj.fullsky_geometry(0.5 * ARCMIN)
    assert "%dx%d" % shape == geom
    nx, ny = shape
    m = torch.ones((ny, nx), dtype=torch.float64, device=dev)
    if mask == "sources":
        radius = max(5 * ARCMIN, 3 * 2 * math.pi / nx)
        zi, zj = R.disk_zeros(wcs, shape, 2000, radius, seed=7)
        m.view(-1)[torch.from_numpy(zj * nx + zi).to(dev)] = 0.0
    else:
        rows = R.band_rows(wcs, shape, 10 * DEG)
        m[torch.from_numpy(rows).to(dev)] = 0.0
        zj = np.concatenate([np.full(nx, rows[0]), np.full(nx, rows[-1])])
        zi = np.concatenate([np.arange(nx), np.arange(nx)])
    _sampled_check(pj, dev, shape, wcs, m, zi, zj, "%s %s" % (geom, mask))


def test_streams_repeat_input_and_overlap(pj, dev):
    """Two calls on two streams with different masks at the same time: each bit-identical to its result alone.  Both calls
    are enqueued through the C entry (which never synchronises) before the host waits once, so they can overlap on the
    device.  A repeated call is bit-identical, the input is unchanged, and an `out` overlapping the input raises."""
    shape, wcs = pj.fullsky_geometry(0.25 * DEG)
    nx, ny = shape
    rng = np.random.default_rng(11)
    maps = []
    for _ in range(2):
        a = np.ones((ny, nx))
        a[rng.integers(0, ny, 50), rng.integers(0, nx, 50)] = 0.0
        maps.append(pj.Enmap(torch.from_numpy(a).to(dev), wcs))
    before = [mm.data.clone() for mm in maps]
    alone = [pj.distance_transform(pj.ExactSeqSDT(), mm).data.clone() for mm in maps]
    torch.cuda.synchronize()
    lib = pj.load_library()
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for _ in range(4):
        outs = [torch.full((ny, nx), float("nan"), dtype=torch.float64, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        for k, st in enumerate((sa, sb)):
            rc = lib.pxl_distance_transform_car_f64(C.byref(wcs.to_struct()), pj._lib.shape_arr(shape),
                                                    C.c_void_p(maps[k].data.data_ptr()), C.c_void_p(outs[k].data_ptr()),
                                                    C.c_void_p(st.cuda_stream))
            assert rc == 0, pj._lib.last_error()
        torch.cuda.synchronize()
        for k in range(2):
            assert bits_equal(outs[k].cpu().numpy(), alone[k].cpu().numpy()), k
    again = pj.distance_transform(pj.ExactSeqSDT(), maps[0]).data
    assert bits_equal(again.cpu().numpy(), alone[0].cpu().numpy())
    for k in range(2):
        assert torch.equal(maps[k].data, before[k])
    big = torch.ones((2 * ny, nx), dtype=torch.float64, device=dev)
    big[0, 0] = 0.0
    src = pj.Enmap(big[:ny], wcs)
    with pytest.raises(ValueError, match="overlaps"):
        pj.distance_transform(pj.ExactSeqSDT(), src, out=pj.Enmap(big[ny // 2:ny // 2 + ny], wcs))
    with pytest.raises(ValueError, match="overlaps"):
        pj.distance_transform(pj.ExactSeqSDT(), src, out=src)


def test_rows_longer_than_one_scan_trip(pj, dev):
    """A 70000-column box (350 degrees of RA at 0.005 degrees, 1094 mask words per row): the row scan runs two trips of 1024
    words and carries its prefix and suffix maxima across them.  Zeros on either side of the trip boundary (word 1024 =
    column 65536), one row with zeros in the first trip only and one with zeros in the second trip only."""
    shape, wcs = _box(pj, 175, -175, 0, 0.015, 0.005)
    nx, ny = shape
    assert shape == (70000, 3) and (nx + 63) // 64 > 1024
    m = np.ones((ny, nx))
    m[0, [100, 69000]] = 0.0
    m[1, [5000, 30000]] = 0.0
    m[2, [66000, 67500]] = 0.0
    _check(_device(pj, dev, m, wcs), m, wcs, "70000 x 3")


def test_non_car_and_3d_maps_are_refused(pj, dev):
    shape, wcs = _box(pj, 20, -20, -10, 10, 0.5)
    nx, ny = shape
    gn = pj.Gnomonic((-0.5, 0.5), (40.0, 20.0), (0.0, 0.0))
    with pytest.raises(ValueError, match="CAR"):
        pj.distance_transform(pj.ExactSeqSDT(), pj.Enmap(torch.zeros((ny, nx), dtype=torch.float64, device=dev), gn))
    with pytest.raises(ValueError, match="2-D"):
        pj.distance_transform(pj.ExactSeqSDT(), pj.Enmap(torch.zeros((2, ny, nx), dtype=torch.float64, device=dev), wcs))


# ---- dense masks, word edges, scan trips, the far hemisphere, limits and refusals ---------------------------------------
# The cases are R.ALL_CASES: tests/test_sdt_ref.py shows on the CPU that the method passes each and names the one-line
# faults of the kernels that each catches.  Every pixel goes through _check with the case's shared brute-force reference.

def _check_case(pj, dev, name, dt=None):
    m, shape, wcs, ref = R.case(pj, name)
    got = _device(pj, dev, m.copy(), wcs, dt)            # the shared mask is read-only; torch wants a writable array
    _check(got, m, wcs, name, ref)
    return got


@pytest.mark.parametrize("mask", R.DENSE_MASKS)
@pytest.mark.parametrize("geom", R.DENSE_GEOMETRIES)
def test_dense_and_structured_masks(pj, dev, geom, mask):
    """Masks of large connected or dense regions of zeros (R.dense_mask) on 4 and 3 degree full-sky CC, 4 degree Fejer1, a
    40 x 20 box and a 300-degree box with DEC running downwards: several zeros per mask word, chains in which every row
    has a point, up to ten pops per push (counted in R.emulate; six on the full-sky maps), rows with and without zeros
    interleaved, ny % 4 = 2, 1, 1, 0 upwards and 3 downwards.
    Worst error / bound measured on the MI355X: 0.345 (full_column on the 300-degree box); per geometry 0.25, 0.26, 0.26,
    0.17, 0.35."""
    _check_case(pj, dev, "dense/%s/%s" % (geom, mask))


def test_dense_masks_all_kinds_same_bits(pj, dev):
    """The three dt kinds give the same bits on every dense mask of the 3 degree full sky."""
    for mask in R.DENSE_MASKS:
        m, shape, wcs, _ = R.case(pj, "dense/cc3/" + mask)
        outs = [_device(pj, dev, m.copy(), wcs, dt) for dt in (pj.ExactSeqSDT(), pj.BruteForceSDT(), pj.ApproxSeqSDT())]
        assert bits_equal(outs[0], outs[1]) and bits_equal(outs[0], outs[2]), mask


@pytest.mark.parametrize("nx", R.WORD_EDGE_NX)
def test_word_edges(pj, dev, nx):
    """nx x 10 boxes of 0.02 degree columns and 5 degree rows, so a row's own zeros decide its pixels and a wrong best column
    shows.  One pattern per row (R.WORD_EDGE_ROWS): zeros on the first and last column, on either side of the word edges
    63 | 64 and 127 | 128, several inside one word with the queries between them, one in the last (partial) word only, a
    full row, an empty row, a random half.  nx = 63 is a single partial word, 64 a single full one; 129 has DEC running
    downwards and 200 RA increasing.  Worst error / bound measured on the MI355X: 0.0017 (the distances are under 4 degrees
    along a row, where the bound's ceiling applies; a wrong column is an error of 1e10 bounds or more, tests/test_sdt_ref.py)."""
    _check_case(pj, dev, "word_edge/%d" % nx)


@pytest.mark.parametrize("case", R.SCAN_TRIP_CASES)
def test_scan_trips(pj, dev, case):
    """The 70000 x 3 geometry (1094 mask words: two trips of the row scans), one row with zeros and two without, so that row
    decides every pixel (R.scan_trip_mask): zeros on the last bit of word 1023 and the first of word 1024, together and
    alone; a zero every 256th column; zeros in words 1024 and above only; one zero on either side of the suffix scan's trip
    edge (words 69 | 70).  Worst error / bound measured on the MI355X: 0.554."""
    _check_case(pj, dev, "scan/" + case)


@pytest.mark.parametrize("case", R.FAR_CASES)
def test_far_hemisphere(pj, dev, case):
    """4 degree full sky with one, two or three zeros (R.far_mask): most pixels lie on the far hemisphere of their nearest
    zero, the chain's points have negative x, and with three rows of zeros a column's chain mixes both signs.
    Worst error / bound measured on the MI355X: 0.366."""
    _check_case(pj, dev, "far/" + case)


def _raw(pj, dev, wcs, shape, src, dst):
    rc = pj.load_library().pxl_distance_transform_car_f64(C.byref(wcs.to_struct()), pj._lib.shape_arr(shape),
                                                          C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    msg = pj._lib.last_error()
    torch.cuda.synchronize()
    return rc, msg


def test_widest_accepted_map(pj, dev):
    """131072 x 2 of exactly 360 degrees: PXL_SDT_MAX_NX columns (2048 mask words, two full scan trips) and the RA limit
    are both accepted, through the C entry into a NaN-filled output and through pj.distance_transform, with the same bits.
    4096 seeded pixels and every zero pixel against the sampled yardstick.  Worst error / bound measured on the MI355X: 0.165."""
    shape, wcs = pj.geometry([[180 * DEG, -180 * DEG], [0.0, 1 * DEG]], (2 * math.pi / 131072, 0.5 * DEG))
    nx, ny = shape
    assert shape == (131072, 2) and nx * abs(wcs.cdelt[0] * wcs.unit) == 2 * math.pi
    rng = np.random.default_rng(131072)
    m = np.ones((ny, nx))
    m[rng.integers(0, ny, 40), rng.integers(0, nx, 40)] = 0.0
    m[0, 0] = m[1, nx - 1] = 0.0
    m[1, [65535, 65536]] = 0.0
    src = torch.from_numpy(m).to(dev)
    dst = torch.full_like(src, float("nan"))
    rc, msg = _raw(pj, dev, wcs, shape, src, dst)
    assert rc == 0, msg
    raw = dst.cpu().numpy()
    assert not np.isnan(raw).any()
    assert bits_equal(raw, _device(pj, dev, m, wcs))
    zj, zi = np.nonzero(m == 0)
    ii = np.concatenate([rng.integers(0, nx, 4096), zi])
    jj = np.concatenate([rng.integers(0, ny, 4096), zj])
    got = raw[jj, ii]
    zero = m[jj, ii] == 0
    assert np.array_equal(got[zero].view(np.int64), np.zeros(int(zero.sum()), np.int64))
    r = R.worst_ratio(got, R.sampled(wcs, shape, ii, jj, zi, zj))
    print("131072 x 2: %d pixels (%d zero), worst error / bound = %.3g" % (ii.size, int(zero.sum()), r))
    assert r <= 1.0


@pytest.mark.parametrize("what", R.REFUSED)
def test_refused_geometries(pj, dev, what):
    """One column more than PXL_SDT_MAX_NX, a top row beyond DEC 90 degrees, 361 columns of 1 degree, and a row step that
    rewind folds back so DEC is not monotone: the C entry returns PXL_EINVAL with the reason in its message and leaves a
    NaN-filled output untouched, bit for bit; pj.distance_transform raises ValueError with the same reason."""
    shape, wcs, reason = R.refused_geometry(pj, what)
    nx, ny = shape
    src = torch.zeros((ny, nx), dtype=torch.float64, device=dev)
    dst = torch.full_like(src, float("nan"))
    before = dst.clone()
    rc, msg = _raw(pj, dev, wcs, shape, src, dst)
    assert rc == -22 and "distance_transform" in msg and reason in msg, (rc, msg)
    assert torch.equal(dst.view(torch.int64), before.view(torch.int64))
    with pytest.raises(ValueError, match=reason):
        pj.distance_transform(pj.ExactSeqSDT(), pj.Enmap(src, wcs))
    with pytest.raises(ValueError, match=reason):
        pj.distance_transform(pj.ExactSeqSDT(), pj.Enmap(src, wcs), out=pj.Enmap(dst, wcs))
    torch.cuda.synchronize()
    assert torch.equal(dst.view(torch.int64), before.view(torch.int64))
