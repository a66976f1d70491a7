"""The host entry points of csrc/pxl_kernels.hip choose a launch shape -- and sometimes another kernel -- from the size, parity
and alignment of a call.  The oracle-checked tests elsewhere run small, torch-aligned calls and so see one side of each choice.
Every test here picks its inputs from the thresholds in the host code so that it takes the OTHER side (the one real maps and
the benchmark run), and compares EVERY output element with a plain reference:

  whole-map writers   posmap of a CAR map is separable (ra[j, i] depends on i only, dec[j, i] on j only): the two vectors come
                      from the CPU oracle, the comparison with their broadcast happens on the device, bit for bit; outputs
                      are pre-filled with NaN so that an element nobody wrote fails.  pixareamap is constant along RA; column
                      0 is held to the oracle's rows within the project's bound 8 eps |cdelt[0] unit| (test_gpu_parity.py).
  streaming kernels   elementwise, so a batch that repeats a block of L = 1 000 003 points (prime, odd) must give the same
                      tiling of the block's result; the block's result is compared with the oracle on the CPU.  An index
                      that wraps, a chunk skipped or written twice lands on a position with another expected value.
  generators          splitmix64 / u01 restated in NumPy uint64 arithmetic from pxl_misc.h.
  refusals            argument checks only: every pointer handed to a refused call covers the full size it describes.

Work items of a 1-D streaming launch: stream_grid() caps the grid at 2^20 blocks of 256 lanes = 2^28 work items (CAP below);
past it the kernels grid-stride.  A batch of CAP * (points per work item) + L points makes the first few thousand blocks take
a second trip, the others one, and leaves the last block partial.

`python tests/test_gpu_launch_paths.py` re-measures the two glibc figures behind the generator bounds (CPU only)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ARCMIN, DEG, GOLDEN, bits_equal

torch = pytest.importorskip("torch")
from gpu_support import to_dev
pytestmark = pytest.mark.gpu

L = 1_000_003                        # block length: prime and odd
CAP = (1 << 20) * 256                # work items of a full stream_grid() launch
EINVAL = -22
TWOPI = 6.283185307179586            # PXL_TWOPI_D
PI = 3.141592653589793               # PXL_PI_D
NAN = float("nan")

# ---- the two measured bounds: glibc double precision against the same formula in long double, on the inputs of the tests below
# (GEN_CASES, GEN_N elements each); `python tests/test_gpu_launch_paths.py` prints them.
#   Box-Muller  v = sqrt(-2 log(1 - u1)) cos(2pi u2).  The argument 2pi * u2 is rounded to double before the cosine: an absolute
#               error of the cosine, which no bound relative to v survives near the zeros of the cosine; it scales with the
#               radius r = sqrt(-2 log(1 - u1)).  The figure is therefore in ulp of r.
#   asin        the argument 2 u2 - 1 is exact in double; the figure is in ulp of the result.
# The device gets the glibc figure plus 4 ulp of the result (its log, cos, sqrt, asin are documented at 1-2 ulp each and the
# formula chains three of them).  Neither figure was taken from the device.
GLIBC_BOXMULLER_ULP_R = 4.304        # measured: the worst case is the rounding of 2pi * u2 (0.5 ulp of an angle near 2pi)
GLIBC_ASIN_ULP = 0.513               # measured
DEVICE_EXTRA_ULP = 4.0
GEN_N = 200_000
GEN_CASES = [(0, 0), (1234, 0), (42, 999_999_937), (7, (1 << 32) + 12_345), (0xDEADBEEFCAFE, (1 << 40) + 3), (99, (1 << 63) + 5)]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pixell_jl_amd as pj
    return pj, pj.load_library(), torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    torch.cuda.empty_cache()


def P(t):
    return C.c_void_p(t.data_ptr())


def S(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def buf(n, dev, offset8=False, dtype=torch.float64, fill=NAN):
    """n elements on the device, 16-byte aligned or (offset8) 8 bytes past a 16-byte boundary; returns (view, owner)"""
    owner = torch.full((n + 2,), fill, dtype=dtype, device=dev)
    assert owner.data_ptr() % 16 == 0
    view = owner[1:n + 1] if offset8 else owner[:n]
    assert view.data_ptr() % 16 == (8 if offset8 else 0)
    return view, owner


def untouched_around(view, owner):
    """the guard elements of buf() still hold NaN"""
    lo = (view.data_ptr() - owner.data_ptr()) // 8
    return bool(torch.isnan(owner[:lo]).all()) and bool(torch.isnan(owner[lo + view.numel():]).all())


def first_bad(got, exp):
    """where two broadcastable tensors differ (NaN counts as different): for the assertion message"""
    bad = torch.nonzero((got != exp).reshape(-1))
    k = int(bad[0]) if bad.numel() else -1
    return "%d elements differ, the first at flat index %d" % (bad.numel(), k)


def bad_rows(got, exp):
    rows = torch.nonzero((got != exp).any(dim=1)).reshape(-1)
    return "%d rows differ: %s ..." % (rows.numel(), rows[:12].tolist())


# ================================================================================================
# 1. whole-map writers
# ================================================================================================

def car(pj, nx, ny):
    """a CAR geometry of any shape: the kernels only see the affine"""
    return (nx, ny), pj.CarClenshawCurtis((-360.0 / nx, 180.0 / (ny - 1)), (nx / 2 + 1.0, (ny + 1) / 2.0), (0.0, 0.0))


def posmap_raw(env, O, shape, wcs, row0, nrows, safe, offset8=False):
    """pxl_posmap_car_f64 into NaN-filled buffers; every element against the oracle's RA and DEC vectors"""
    pj, lib, dev = env
    nx, ny = shape
    ra, keep_a = buf(nrows * nx, dev, offset8)
    dec, keep_d = buf(nrows * nx, dev, offset8)
    w = wcs.to_struct()
    rc = lib.pxl_posmap_car_f64(C.byref(w), pj._lib.shape_arr(shape), row0, nrows, P(ra), P(dec), int(safe), S(dev))
    assert rc == 0, pj._lib.last_error()
    ra_vec = to_dev(O.posmap(wcs, (nx, ny), row0=row0, nrows=1, safe=safe)[0][0], dev)
    dec_vec = to_dev(O.posmap(wcs, (1, ny), row0=row0, nrows=nrows, safe=safe)[1][:, 0], dev)
    assert untouched_around(ra, keep_a) and untouched_around(dec, keep_d)
    ra, dec = ra.view(nrows, nx), dec.view(nrows, nx)
    tag = (shape, row0, nrows, safe, offset8)
    assert torch.equal(ra, ra_vec.expand_as(ra)), (tag, "ra", bad_rows(ra, ra_vec))
    assert torch.equal(dec, dec_vec[:, None].expand_as(dec)), (tag, "dec", bad_rows(dec, dec_vec[:, None]))


@pytest.mark.parametrize("safe", [True, False])
def test_posmap_fronts8_fullsky_every_pixel(env, O, safe):
    """43200 x 21601: nych = ceil(21601 / 32) = 676 row chunks >= 16 * 8 = 128, so fronts = 8; per = ceil(676 / 8) = 85,
    grid.y = 680, and the last front has 4 idle chunk slots (jr0 >= nrows).  Aligned, even nx: 16-byte stores."""
    pj = env[0]
    shape, wcs = pj.fullsky_geometry(2 * math.pi / 43200)
    assert shape == (43200, 21601)
    posmap_raw(env, O, shape, wcs, 0, shape[1], safe)


@pytest.mark.parametrize("safe", [True, False])
def test_posmap_fronts8_row_window(env, O, safe):
    """row0 = 4099, nrows = 4100 + 13 of the 43200 x 21601 geometry: nych = ceil(4113 / 32) = 129 >= 128, so fronts = 8;
    per = 17, grid.y = 136, 7 idle slots; the last chunk holds 17 rows.  DEC must be that of map rows row0 + jr."""
    pj = env[0]
    shape, wcs = pj.fullsky_geometry(2 * math.pi / 43200)
    posmap_raw(env, O, shape, wcs, 4099, 4100 + 13, safe)


def test_posmap_fronts8_odd_nx_row0_unsafe(env, O):
    """Odd nx = 4321 with 4131 rows: nych = 130 >= 128, fronts = 8, per = 17 (6 idle slots); odd nx takes the element-wise
    stores (vec = false) and the last lane of a row writes one pixel.  The whole map with safe = 1, then row0 = 7 with
    nrows = 4110 (nych = 129, still fronts = 8) and safe = 0."""
    pj = env[0]
    shape, wcs = car(pj, 4321, 4131)
    posmap_raw(env, O, shape, wcs, 0, 4131, True)
    posmap_raw(env, O, shape, wcs, 7, 4110, False)


def test_posmap_unaligned_outputs_even_nx(env, O):
    """ra and dec 8 bytes past a 16-byte boundary with even nx: k_posmap_car's `vec` is false although nx is even (element-wise
    stores).  1000 x 4200 (nych = 132: fronts = 8, per = 17) and 360 x 181 (nych = 6: fronts = 1), both safe values; then a
    window (row0 = 33, 4100 rows: nych = 129, fronts = 8)."""
    pj = env[0]
    for shape, wcs in (car(pj, 1000, 4200), pj.fullsky_geometry(1 * DEG)):
        for safe in (True, False):
            posmap_raw(env, O, shape, wcs, 0, shape[1], safe, offset8=True)
    shape, wcs = car(pj, 1000, 4200)
    posmap_raw(env, O, shape, wcs, 33, 4100, True, offset8=True)


def test_posmap_grid_limit_falls_back_to_one_front(env, O):
    """2 columns, 65535 * 32 - 5 = 2 097 115 rows: nych = 65535, per = ceil(65535 / 8) = 8192 and per * fronts = 65536 > 65535,
    so the launch falls back to fronts = 1 with grid.y = 65535 (34 MB per output)."""
    pj = env[0]
    shape, wcs = car(pj, 2, 65535 * 32 - 5)
    posmap_raw(env, O, shape, wcs, 0, shape[1], True)


def test_posmap_refuses_more_rows_than_the_grid_holds(env):
    """65535 * 32 + 1 rows in one call: PXL_EINVAL with the limit in the message, outputs untouched.  The buffers cover the
    whole request.  One row fewer (nych = 65535: one front) is the largest call there is."""
    pj, lib, dev = env
    ny = 65535 * 32 + 1
    shape, wcs = car(pj, 1, ny)
    ra, _a = buf(ny, dev)
    dec, _d = buf(ny, dev)
    w = wcs.to_struct()
    rc = lib.pxl_posmap_car_f64(C.byref(w), pj._lib.shape_arr(shape), 0, ny, P(ra), P(dec), 1, S(dev))
    assert rc == EINVAL
    assert str(65535 * 32) in pj._lib.last_error(), pj._lib.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(ra).all()) and bool(torch.isnan(dec).all())
    rc = lib.pxl_posmap_car_f64(C.byref(w), pj._lib.shape_arr(shape), 1, ny - 1, P(ra), P(dec), 1, S(dev))
    assert rc == 0, pj._lib.last_error()
    assert bool(torch.isfinite(ra[:ny - 1]).all()) and bool(torch.isnan(ra[ny - 1:]).all())
    assert bool(torch.isfinite(dec[:ny - 1]).all()) and bool(torch.isnan(dec[ny - 1:]).all())


def pixarea_raw(env, shape, wcs, row0, nrows, offset8=False):
    pj, lib, dev = env
    nx = shape[0]
    area, keep = buf(nrows * nx, dev, offset8)
    w = wcs.to_struct()
    rc = lib.pxl_pixareamap_car_f64(C.byref(w), pj._lib.shape_arr(shape), row0, nrows, P(area), S(dev))
    assert rc == 0, pj._lib.last_error()
    assert untouched_around(area, keep)
    return area.view(nrows, nx)


def pixarea_check(O, shape, wcs, area, row0=0):
    """constant along RA over the whole map (bit for bit); column 0 within 8 eps |cdelt[0] unit| of the oracle's rows"""
    assert torch.equal(area, area[:, :1].expand_as(area)), ((shape, row0), bad_rows(area, area[:, :1]))
    col = area[:, 0].cpu().numpy()
    assert not np.isnan(col).any(), ((shape, row0), "rows never written", np.flatnonzero(np.isnan(col))[:12])
    ref = O.pixarea_rows(wcs, shape[1])[row0:row0 + area.shape[0]]
    err = np.abs(col - ref)
    bound = 8 * np.finfo(float).eps * abs(wcs.cdelt[0] * wcs.unit)
    assert err.max() < bound, ((shape, row0), int(np.argmax(err)), float(err.max()), bound)


def test_pixareamap_chunks_fronts8_fullsky(env, O):
    """43200 x 21601, aligned: total = 21600 * 21601 pairs = 113 912 chunks of 4096 pairs >= 64 * 8 = 512, so fronts = 8 and
    per = 14239.  A row is 21600 pairs = 5.27 chunks: nearly every chunk spans a row boundary (the `while (t >= next)` walk).
    Then a window of the same geometry (row0 = 4099, 10 000 rows: 52 735 chunks, fronts = 8, per = 6592, 1 idle slot), which
    must equal the same rows of the full call bit for bit."""
    pj = env[0]
    shape, wcs = pj.fullsky_geometry(2 * math.pi / 43200)
    full = pixarea_raw(env, shape, wcs, 0, shape[1])
    pixarea_check(O, shape, wcs, full)
    win = pixarea_raw(env, shape, wcs, 4099, 10000)
    assert torch.equal(win, full[4099:14099]), bad_rows(win, full[4099:14099])


def test_pixareamap_chunks_idle_slots_and_row_windows(env, O):
    """3002 x 1403, aligned: nx / 2 = 1501 pairs per row does not divide 4096; total = 2 105 903 pairs = 515 chunks >= 512, so
    fronts = 8, per = 65, 520 blocks: 5 idle slots, and the last chunk is partial.  Windows through the C ABI: (5, 1395)
    is 512 chunks (fronts = 8, per = 64, none idle), (700, 703) is 258 chunks (fronts = 1); each equals the rows of the full
    call bit for bit.  The same windows on the row path (k_pixareamap_car: the map 8 bytes off) give the same bits again."""
    pj = env[0]
    shape, wcs = car(pj, 3002, 1403)
    full = pixarea_raw(env, shape, wcs, 0, shape[1])
    pixarea_check(O, shape, wcs, full)
    for row0, nrows in ((5, 1395), (700, 703), (1402, 1), (0, 1)):
        win = pixarea_raw(env, shape, wcs, row0, nrows)
        assert torch.equal(win, full[row0:row0 + nrows]), (row0, nrows, bad_rows(win, full[row0:row0 + nrows]))
        win = pixarea_raw(env, shape, wcs, row0, nrows, offset8=True)
        assert torch.equal(win, full[row0:row0 + nrows]), ("row path", row0, nrows, bad_rows(win, full[row0:row0 + nrows]))


def test_pixareamap_rows_two_launches_odd_nx(env, O):
    """Odd nx = 3 with 70 001 rows: k_pixareamap_car takes one row per blockIdx.y, 65535 per launch, so rows 65535 .. 70000 come
    from a second launch at area + 65535 * nx with row0 + 65535.  A window (row0 = 11, 69 985 rows: two launches again, the
    second starting at map row 65546) equals the rows of the full call."""
    pj = env[0]
    shape, wcs = car(pj, 3, 70001)
    full = pixarea_raw(env, shape, wcs, 0, shape[1])
    pixarea_check(O, shape, wcs, full)
    win = pixarea_raw(env, shape, wcs, 11, 69985)
    assert torch.equal(win, full[11:11 + 69985]), bad_rows(win, full[11:11 + 69985])
    pixarea_check(O, shape, wcs, win, row0=11)


def test_pixareamap_unaligned_even_nx_and_reference_data(env, O, literals):
    """An even-nx map written 8 bytes off a 16-byte boundary leaves the chunk kernel for k_pixareamap_car with element-wise
    stores.  1000 x 4200 both ways (aligned: 513 chunks, fronts = 8, per = 65, 7 idle slots); then the reference's two data
    files (tests/golden) held to the bounds of reference_literals.json on both paths."""
    pj, lib, dev = env
    shape, wcs = car(pj, 1000, 4200)
    off = pixarea_raw(env, shape, wcs, 0, shape[1], offset8=True)
    pixarea_check(O, shape, wcs, off)
    ali = pixarea_raw(env, shape, wcs, 0, shape[1])
    assert torch.equal(off, ali), bad_rows(off, ali)
    for lit in literals["pixareamap"]:
        if lit["kind"] == "fullsky_1deg":
            shape, wcs = pj.fullsky_geometry(1 * DEG)
        else:
            b = lit["box_deg"]
            shape, wcs = pj.geometry([[b[0][0] * DEG, b[0][1] * DEG], [b[1][0] * DEG, b[1][1] * DEG]], lit["res_arcmin"] * ARCMIN)
        ref = np.loadtxt(os.path.join(GOLDEN, lit["file"]))
        for offset8 in (False, True):
            area = pixarea_raw(env, shape, wcs, 0, shape[1], offset8=offset8)
            pixarea_check(O, shape, wcs, area)
            assert np.abs(area[:, 0].cpu().numpy() - ref).sum() < lit["tol_sum_abs"], (lit["src"], offset8)


# ================================================================================================
# 2. grid-stride trips of the streaming kernels
# ================================================================================================

def tiled(block, n):
    """(n, ...) tensor that repeats the (L, ...) block: k whole copies and a tail"""
    k, tail = divmod(n, L)
    rest = tuple(block.shape[1:])
    out = torch.empty((n,) + rest, dtype=block.dtype, device=block.device)
    out[:k * L].view((k, L) + rest).copy_(block.unsqueeze(0).expand((k, L) + rest))
    out[k * L:].copy_(block[:tail])
    return out


def assert_tiled(out, blk, tag):
    """every element of `out` against the tiling of the block's result"""
    n = out.shape[0]
    k, tail = divmod(n, L)
    assert k >= 2 and blk.shape[0] == L and tuple(out.shape[1:]) == tuple(blk.shape[1:])
    rest = tuple(blk.shape[1:])
    body, exp = out[:k * L].view((k, L) + rest), blk.unsqueeze(0).expand((k, L) + rest)
    assert torch.equal(body, exp), (tag, first_bad(body, exp))
    assert torch.equal(out[k * L:], blk[:tail]), (tag, "tail", first_bad(out[k * L:], blk[:tail]))


def pix_block(rng, shape):
    return np.stack([rng.uniform(-2.5 * shape[0], 3.5 * shape[0], L), rng.uniform(-2.5 * shape[1], 3.5 * shape[1], L)], axis=1)


def sky_block(rng):
    """on-sky angles and angles many periods away"""
    ra = np.concatenate([rng.uniform(-math.pi, math.pi, L // 2), rng.uniform(-40 * math.pi, 40 * math.pi, L - L // 2)])
    dec = np.concatenate([rng.uniform(-math.pi / 2, math.pi / 2, L // 2), rng.uniform(-17 * math.pi, 17 * math.pi, L - L // 2)])
    p = rng.permutation(L)
    return np.stack([ra[p], dec[p]], axis=1)


def test_stream_pix2sky_affine_two_trips(env, O):
    """pj.pix2sky(safe=False) -> k_pix2sky_pairs<1>, one point per work item: n = 2^28 + L points is 1 052 483 blocks of 256 >
    2^20, so the grid is capped and blocks 0 .. 3906 take a second trip (k0 += 2^28); byte offsets pass 2^32."""
    pj, lib, dev = env
    shape, wcs = pj.fullsky_geometry(1 * DEG)
    blk = pix_block(np.random.default_rng(11), shape)
    d_blk = to_dev(blk, dev)
    r_blk = pj.pix2sky((shape, wcs), d_blk, safe=False)
    assert bits_equal(r_blk.cpu().numpy(), O.pix2sky(wcs, blk, O.WRAP_NONE))
    n = CAP + L
    out = pj.pix2sky((shape, wcs), tiled(d_blk, n), safe=False)
    assert_tiled(out, r_blk, "pix2sky safe=False")


def test_stream_pix2sky_rewind_two_trips(env, O):
    """pj.pix2sky_rewind -> k_pix2sky_pairs<2>, two points per work item (chunks of 512 per block): n = 2^29 + L points is
    (n + 1) / 2 = 2^28 + 500 002 work items > 2^28, so the first 1954 blocks take a second trip (k0 += 2^29)."""
    pj, lib, dev = env
    shape, wcs = pj.fullsky_geometry(1 * DEG)
    blk = pix_block(np.random.default_rng(12), shape)
    d_blk = to_dev(blk, dev)
    r_blk = pj.pix2sky_rewind((shape, wcs), d_blk)
    assert bits_equal(r_blk.cpu().numpy(), O.pix2sky(wcs, blk, O.WRAP_REWIND))
    n = 2 * CAP + L
    out = pj.pix2sky_rewind((shape, wcs), tiled(d_blk, n))
    assert_tiled(out, r_blk, "pix2sky_rewind")


@pytest.mark.parametrize("safe", [True, False])
def test_stream_sky2pix_two_trips(env, O, safe):
    """pj.sky2pix on a 2xN batch: safe=True -> k_sky2pix_pairs<2> (n = 2^29 + L points, 2^28 + 500 002 work items); safe=False
    -> k_sky2pix_pairs<1> (n = 2^28 + L).  Both pass the 2^20-block cap, by 1954 and 3907 blocks."""
    pj, lib, dev = env
    shape, wcs = pj.fullsky_geometry(1 * DEG)
    blk = sky_block(np.random.default_rng(13 + safe))
    d_blk = to_dev(blk, dev)
    r_blk = pj.sky2pix((shape, wcs), d_blk, safe=safe)
    assert bits_equal(r_blk.cpu().numpy(), O.sky2pix(wcs, shape, blk, safe=safe, form=O.FORM_RECIP))
    n = (2 * CAP if safe else CAP) + L
    out = pj.sky2pix((shape, wcs), tiled(d_blk, n), safe=safe)
    assert_tiled(out, r_blk, "sky2pix safe=%s" % safe)


def soa_call(env, fn, a, b, extra, offset8):
    """one SoA entry through the C ABI: inputs a, b (views of equal length), two NaN-filled outputs with the same alignment"""
    pj, lib, dev = env
    n = a.numel()
    x, kx = buf(n, dev, offset8)
    y, ky = buf(n, dev, offset8)
    rc = fn(n, P(a), P(b), P(x), P(y), *extra)
    assert rc == 0, pj._lib.last_error()
    assert untouched_around(x, kx) and untouched_around(y, ky)
    return x, y


def soa_inputs(env, cols, n, offset8):
    """the two columns of a block as (block views, tiled views of length n), all with the wanted alignment"""
    dev = env[2]
    out = []
    for c in cols:
        small, _ = buf(L, dev, offset8)
        small.copy_(to_dev(c, dev))
        big, _ = buf(n, dev, offset8)
        big.copy_(tiled(small, n))
        out.append((small, big))
    return out


@pytest.mark.parametrize("offset8", [False, True])
def test_stream_soa_forms_two_trips(env, O, offset8):
    """The SoA pix2sky / sky2pix forms take two adjacent points per work item: n = 2^29 + L points is 2^28 + 500 002 work items,
    past the cap.  n is odd: the last work item holds one point.  Aligned: 16-byte accesses (vec = 1); with the four arrays
    8 bytes past a 16-byte boundary: element-wise accesses (vec = 0).  pix2sky runs with safe = 1 aligned and 0 offset, sky2pix
    with safe = 0 aligned and 1 offset (both pairings run at small sizes in test_gpu_parity.py)."""
    pj, lib, dev = env
    shape, wcs = pj.fullsky_geometry(1 * DEG)
    w, shp, st = wcs.to_struct(), pj._lib.shape_arr(shape), S(dev)
    n = 2 * CAP + L
    rng = np.random.default_rng(15)
    # pix2sky
    pb = pix_block(rng, shape)
    safe = not offset8
    ea, ed = O.pix2sky_soa(wcs, pb[:, 0], pb[:, 1], safe=safe)
    (ba, a), (bb, b) = soa_inputs(env, (pb[:, 0], pb[:, 1]), n, offset8)

    def p2s(n_, a_, b_, x_, y_, *e):
        return lib.pxl_pix2sky_car_soa_f64(C.byref(w), n_, a_, b_, x_, y_, *e)
    xb, yb = soa_call(env, p2s, ba, bb, (int(safe), st), offset8)
    assert bits_equal(xb.cpu().numpy(), ea) and bits_equal(yb.cpu().numpy(), ed)
    x, y = soa_call(env, p2s, a, b, (int(safe), st), offset8)
    assert_tiled(x, xb, "pix2sky SoA ra")
    assert_tiled(y, yb, "pix2sky SoA dec")
    del x, y, a, b
    # sky2pix (the rounding of the broadcast form, FORM_RECIP_AV, as pj.sky2pix(m, ra, dec) calls it)
    sb = sky_block(rng)
    safe = offset8
    ex, ey = O.sky2pix_soa(wcs, shape, sb[:, 0], sb[:, 1], safe=safe, form=O.FORM_RECIP_AV)
    (ba, a), (bb, b) = soa_inputs(env, (sb[:, 0], sb[:, 1]), n, offset8)

    def s2p(n_, a_, b_, x_, y_, *e):
        return lib.pxl_sky2pix_car_soa_f64(C.byref(w), shp, n_, a_, b_, x_, y_, *e)
    xb, yb = soa_call(env, s2p, ba, bb, (int(safe), pj._lib.FORM_RECIP_AV, st), offset8)
    assert bits_equal(xb.cpu().numpy(), ex) and bits_equal(yb.cpu().numpy(), ey)
    x, y = soa_call(env, s2p, a, b, (int(safe), pj._lib.FORM_RECIP_AV, st), offset8)
    assert_tiled(x, xb, "sky2pix SoA x")
    assert_tiled(y, yb, "sky2pix SoA y")


def test_stream_gnomonic_two_trips(env):
    """Gnomonic pix2sky / sky2pix on vectors -> k_tan_points, two points per work item: n = 2^29 + L points is 2^28 + 500 002
    work items.  The block's result is held to the per-point bounds of test_gpu_gnomonic_accuracy.py against the long double
    yardstick; the tiling of that result is exact (the same evaluator per element, whatever the trip)."""
    import gnomonic_ref as G
    from test_gpu_gnomonic_accuracy import _scatter, check_pix2sky, check_sky2pix
    pj, lib, dev = env
    assert np.finfo(np.longdouble).eps < 2e-19, "the yardstick needs a long double wider than double"
    rng = np.random.default_rng(16)
    wcs = pj.Gnomonic((-1.0 / 60, 1.0 / 60), (1000.5, 900.5), (25.0, 35.0))
    shape = (2000, 1800)
    n = 2 * CAP + L
    ii, jj = _scatter(wcs, rng, L, max_deg=80.0)
    di, dj = to_dev(ii, dev), to_dev(jj, dev)
    ra_b, dec_b = pj.pix2sky((shape, wcs), di, dj)
    check_pix2sky("pix2sky block", wcs, ii, jj, ra_b.cpu().numpy(), dec_b.cpu().numpy())
    big_i, big_j = tiled(di, n), tiled(dj, n)
    ra, dec = pj.pix2sky((shape, wcs), big_i, big_j)
    assert_tiled(ra, ra_b, "Gnomonic pix2sky ra")
    assert_tiled(dec, dec_b, "Gnomonic pix2sky dec")
    del ra, dec
    tra, tdec = G.tan_pix2sky(wcs, ii, jj)
    sra, sdec = tra.astype(np.float64), tdec.astype(np.float64)
    da, dd = to_dev(sra, dev), to_dev(sdec, dev)
    x_b, y_b = pj.sky2pix((shape, wcs), da, dd)
    check_sky2pix("sky2pix block", wcs, sra, sdec, x_b.cpu().numpy(), y_b.cpu().numpy())
    big_i.copy_(tiled(da, n))
    big_j.copy_(tiled(dd, n))
    x, y = pj.sky2pix((shape, wcs), big_i, big_j)
    assert_tiled(x, x_b, "Gnomonic sky2pix x")
    assert_tiled(y, y_b, "Gnomonic sky2pix y")


def test_stream_rewind_two_trips(env, O):
    """pj.rewind_ -> k_rewind, four values per work item: n = 2^30 + L values is 2^28 + 250 001 work items, past the cap; in
    place, with a period and a reference angle of their own."""
    pj, lib, dev = env
    rng = np.random.default_rng(17)
    blk = rng.uniform(-300.0, 300.0, L)
    period, ref = 2.5, 0.75
    d_blk = to_dev(blk, dev)
    r_blk = pj.rewind_(d_blk.clone(), period, ref)
    exp = blk.copy()
    O.lib().pxl_rewind_array_cpu(C.c_int64(L), C.c_int64(1), exp.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(period), C.c_double(ref))
    assert bits_equal(r_blk.cpu().numpy(), exp) and bits_equal(exp[:3], [O.rewind(v, period, ref) for v in blk[:3]])
    n = 4 * CAP + L
    big = tiled(d_blk, n)
    pj.rewind_(big, period, ref)
    assert_tiled(big, r_blk, "rewind_")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_stream_sample_bilinear_two_trips(env, O, dtype):
    """pj.sample_bilinear, direct (k_sample_bilinear) and through SamplePairs (k_sample_pairs): PXL_SUNR = 4 points per work
    item, so n = 2^30 + L points is 2^28 + 250 001 work items, past the cap.  17 GB of coordinates and 8.6 GB (f64) of output
    at once; the source is the 360 x 181 full-sky map, which the oracle samples at the block's points."""
    pj, lib, dev = env
    shape, wcs = pj.fullsky_geometry(1 * DEG)
    nx, ny = shape
    rng = np.random.default_rng(18)
    src = rng.normal(size=(ny, nx))
    sky = np.stack([rng.uniform(-math.pi, math.pi, L), np.arcsin(rng.uniform(-1, 1, L))], axis=1)
    if dtype == "f32":
        src = src.astype(np.float32)
        exp = O.sample_bilinear_f32(wcs, (nx, ny, 1), src[None], sky)
        m = pj.Enmap(to_dev(src, dev, np.float32), wcs)
    else:
        exp = O.sample_bilinear(wcs, (nx, ny, 1), src[None], sky)
        m = pj.Enmap(to_dev(src, dev), wcs)
    d_sky = to_dev(sky, dev)
    pairs = pj.SamplePairs(m)
    r_blk = pj.sample_bilinear(m, d_sky)
    assert np.array_equal(r_blk.cpu().numpy(), exp) and not np.isnan(exp).any()
    assert torch.equal(pj.sample_bilinear(None, d_sky, pairs=pairs), r_blk)
    n = 4 * CAP + L
    big = tiled(d_sky, n)
    out = pj.sample_bilinear(m, big)
    assert out.shape == (1, n)
    assert_tiled(out[0], r_blk[0], "sample_bilinear " + dtype)
    del out
    out = pj.sample_bilinear(None, big, pairs=pairs)
    assert_tiled(out[0], r_blk[0], "sample_bilinear pairs " + dtype)


def test_stream_fits_swaps_two_trips(env):
    """pxl_fits_encode_f64 (k_f64_to_be), pxl_fits_decode_f64 with BITPIX -64 and -32 (k_bswap_to_f64) and pxl_fits_swap_f32
    (k_bswap32) take four elements per work item: n = 2^30 + L elements is 2^28 + 250 001 work items, past the cap.  The
    reference of the block is numpy.ndarray.byteswap; values are compared as integers (every bit pattern, NaNs included)."""
    pj, lib, dev = env
    rng = np.random.default_rng(19)
    n = 4 * CAP + L
    st = S(dev)
    blk = rng.integers(-2**63, 2**63 - 1, L, dtype=np.int64)            # any bit pattern as a Float64
    d_blk = to_dev(blk, dev, np.int64)
    swapped = to_dev(blk.byteswap(), dev, np.int64)
    src = tiled(d_blk, n)
    raw = torch.zeros(n, dtype=torch.int64, device=dev)
    assert lib.pxl_fits_encode_f64(P(src), P(raw), n, st) == 0, pj._lib.last_error()
    assert_tiled(raw, swapped, "fits_encode_f64")
    src.zero_()
    assert lib.pxl_fits_decode_f64(P(raw), P(src), n, -64, st) == 0, pj._lib.last_error()
    assert_tiled(src, d_blk, "fits_decode_f64 BITPIX -64")
    del raw
    # BITPIX -32: big-endian IEEE single, widened exactly
    f32 = rng.normal(size=L).astype(np.float32)
    f32[:4] = [0.0, -0.0, 1.5, 3.4e38]
    be32 = to_dev(f32.view(np.int32).byteswap(), dev, np.int32)
    raw32 = tiled(be32, n)
    assert lib.pxl_fits_decode_f64(P(raw32), P(src), n, -32, st) == 0, pj._lib.last_error()
    assert_tiled(src, to_dev(f32.astype(np.float64).view(np.int64), dev, np.int64), "fits_decode_f64 BITPIX -32")
    del src
    out32 = torch.zeros(n, dtype=torch.int32, device=dev)
    assert lib.pxl_fits_swap_f32(P(raw32), P(out32), n, st) == 0, pj._lib.last_error()
    assert_tiled(out32, to_dev(f32.view(np.int32), dev, np.int32), "fits_swap_f32")


# k_rewind and the three FITS swaps carry four elements per lane: a block's trip is 256 * 4 = 1024 elements.  One element, one
# short of a wave row of the block (every lane's later three guarded off), and one either side of a full trip (the last lane's
# last element missing; a second block with one element).
TAILS = [1, 255, 1023, 1025]
SLACK = 64                           # elements after the output that no call may write


@pytest.mark.parametrize("n", TAILS)
def test_stream_rewind_tail(env, O, n):
    """pj.rewind_ in place on the first n of n + SLACK values: the n equal the oracle's, the slack (values a rewind would move)
    keeps its bits."""
    pj, lib, dev = env
    rng = np.random.default_rng(170 + n)
    blk = rng.uniform(-300.0, 300.0, n + SLACK)
    period, ref = 2.5, 0.75
    d_all = to_dev(blk, dev)
    pj.rewind_(d_all[:n], period, ref)
    exp = blk.copy()
    O.lib().pxl_rewind_array_cpu(C.c_int64(n), C.c_int64(1), exp.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(period), C.c_double(ref))
    assert not bits_equal(exp[:n], blk[:n])
    assert bits_equal(d_all.cpu().numpy(), exp)


@pytest.mark.parametrize("n", TAILS)
def test_stream_fits_swaps_tail(env, n):
    """pxl_fits_encode_f64, pxl_fits_decode_f64 (BITPIX -64 and -32) and pxl_fits_swap_f32 on n elements against
    numpy.ndarray.byteswap, as integers; SLACK sentinel elements after each output keep their bits."""
    pj, lib, dev = env
    rng = np.random.default_rng(190 + n)
    st = S(dev)
    sent64, sent32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A

    def out(dtype, sentinel):
        return torch.full((n + SLACK,), sentinel, dtype=dtype, device=dev)

    def check(got, exp, sentinel, what):
        got = got.cpu().numpy()
        assert np.array_equal(got[:n], exp), what
        assert (got[n:] == sentinel).all(), what + ": wrote past n"

    blk = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)            # any bit pattern as a Float64
    raw = out(torch.int64, sent64)
    assert lib.pxl_fits_encode_f64(P(to_dev(blk, dev, np.int64)), P(raw), n, st) == 0, pj._lib.last_error()
    check(raw, blk.byteswap(), sent64, "fits_encode_f64")
    back = out(torch.int64, sent64)
    assert lib.pxl_fits_decode_f64(P(raw), P(back), n, -64, st) == 0, pj._lib.last_error()
    check(back, blk, sent64, "fits_decode_f64 BITPIX -64")
    f32 = rng.normal(size=n).astype(np.float32)
    f32[0] = -0.0
    be32 = to_dev(f32.view(np.int32).byteswap(), dev, np.int32)
    wide = out(torch.int64, sent64)
    assert lib.pxl_fits_decode_f64(P(be32), P(wide), n, -32, st) == 0, pj._lib.last_error()
    check(wide, f32.astype(np.float64).view(np.int64), sent64, "fits_decode_f64 BITPIX -32")
    out32 = out(torch.int32, sent32)
    assert lib.pxl_fits_swap_f32(P(be32), P(out32), n, st) == 0, pj._lib.last_error()
    check(out32, f32.view(np.int32), sent32, "fits_swap_f32")


def test_pix2sky_unwind_fused_above_onepass_limit(env, O):
    """pj.pix2sky(safe=True), out of place, n = 2^29 + L >= PXL_UW_ONEPASS_MAX = 2^29: the one-pass kernel is not taken and
    unwind_fused (k_unwind_sums<UwSrcPix2> -> k_scan_wsums -> k_unwind_apply) runs instead.  Not elementwise, so by definition
    (oracle: y[k] = m[k] - rint((m[k] - y[k-1]) / 2pi) * 2pi with m = rewind(affine)), over all points on the device:
      * out - m is an integer multiple c of 2pi within one ulp of the product fl(c * 2pi) -- and, the oracle's single rounding
        restated, out == fl(m + fl(c * 2pi)) bit for bit;
      * |out[k] - out[k-1]| <= pi along each coordinate row;  out[0] == m[0];
      * the first and the last 100 000 points equal the oracle's sequential recurrence (the last started from out[n - 100001])."""
    pj, lib, dev = env
    shape, wcs = pj.fullsky_geometry(1 * DEG)
    W = 100_000
    n = 2 * CAP + L
    blk = pix_block(np.random.default_rng(20), shape)
    inp = tiled(to_dev(blk, dev), n)
    out = pj.pix2sky((shape, wcs), inp, safe=True)
    assert out.data_ptr() != inp.data_ptr()
    m = pj.pix2sky_rewind((shape, wcs), inp)                    # elementwise; its own tiling is tested above
    head_in, tail_in = inp[:W].cpu().numpy(), inp[n - W:].cpu().numpy()
    del inp
    assert torch.equal(out[0], m[0])
    # the oracle's recurrence on the two windows
    head = out[:W].cpu().numpy()
    assert bits_equal(head, O.pix2sky(wcs, head_in, O.WRAP_UNWIND))
    tail, prev = out[n - W:].cpu().numpy(), out[n - W - 1].cpu().numpy()
    m_tail = O.pix2sky(wcs, tail_in, O.WRAP_REWIND)
    assert bits_equal(m[n - W:].cpu().numpy(), m_tail)
    exp = np.empty_like(m_tail)
    period = np.float64(TWOPI)
    for col in range(2):
        y = np.float64(prev[col])
        mm = m_tail[:, col]
        for k in range(W):
            y = mm[k] - np.rint((mm[k] - y) / period) * period
            exp[k, col] = y
    assert bits_equal(tail, exp)
    # every point: steps of at most pi, and an integer number of turns away from the rewound value
    step = torch.diff(out, dim=0).abs_().max().item()
    assert step <= math.pi, step
    d = out - m
    prod = (d / TWOPI).round_().mul_(TWOPI)                     # fl(c * 2pi)
    assert torch.equal(out, m + prod), first_bad(out, m + prod)
    del m
    d.sub_(prod).abs_()
    prod.abs_()
    ulp = torch.nextafter(prod, torch.full((), float("inf"), dtype=torch.float64, device=dev)).sub_(prod)
    print("unwind, %d points: |out| up to %.1f rad, c up to %d turns" % (n, out.abs().max().item(), round(prod.max().item() / TWOPI)))
    assert bool((d <= ulp).all()), first_bad(d, torch.minimum(d, ulp))


# ================================================================================================
# 3. the generators, against NumPy
# ================================================================================================

def splitmix64(z):
    """pxl_misc.h: splitmix64 in uint64 array arithmetic (wraps modulo 2^64)"""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def u01(bits):
    return (bits >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def uniforms(seed, offset, n):
    """(u1, u2) of counters offset .. offset + n - 1 (k_fill_random / k_fill_sphere)"""
    ctr = np.arange(n, dtype=np.uint64) + np.uint64(offset)
    s = np.uint64(seed)
    u1 = u01(splitmix64(s ^ splitmix64(np.uint64(2) * ctr)))
    u2 = u01(splitmix64(s ^ splitmix64(np.uint64(2) * ctr + np.uint64(1))))
    return u1, u2


def boxmuller_ld(u1, u2):
    """the Box-Muller formula of k_fill_random in long double: returns (value, radius)"""
    ld = np.longdouble
    r = np.sqrt(ld(-2.0) * np.log(ld(1.0) - u1.astype(ld)))
    return r * np.cos(ld(TWOPI) * u2.astype(ld)), r


def test_fill_random_uniform_matches_numpy(env):
    """kind = 1: u01(splitmix64(seed ^ splitmix64(2 ctr))) with ctr = k + offset, bit for bit, offsets beyond 2^32 and 2^63
    (2 * ctr wraps in uint64, as on the device) included."""
    pj, lib, dev = env
    for seed, offset in GEN_CASES:
        t = torch.full((GEN_N,), NAN, dtype=torch.float64, device=dev)
        pj.fill_random_(t, seed, offset, kind="uniform")
        u1, _ = uniforms(seed, offset, GEN_N)
        assert bits_equal(t.cpu().numpy(), u1), (seed, offset)
        assert 0.0 <= u1.min() and u1.max() < 1.0


def test_fill_random_normal_against_long_double(env):
    """kind = 0: sqrt(-2 log(1 - u1)) cos(2pi u2) through the device's log, sqrt, cos, against the same formula in long double:
    |err| <= GLIBC_BOXMULLER_ULP_R ulp(r) + 4 ulp(value) (see the constants at the top)."""
    pj, lib, dev = env
    assert np.finfo(np.longdouble).eps < 2e-19
    for seed, offset in GEN_CASES:
        t = torch.full((GEN_N,), NAN, dtype=torch.float64, device=dev)
        pj.fill_random_(t, seed, offset, kind="normal")
        got = t.cpu().numpy()
        ref, r = boxmuller_ld(*uniforms(seed, offset, GEN_N))
        err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        bound = GLIBC_BOXMULLER_ULP_R * np.spacing(r.astype(np.float64)) + DEVICE_EXTRA_ULP * np.spacing(np.abs(ref.astype(np.float64)))
        q = err / bound
        k = int(np.argmax(q))
        print("fill_random normal seed %d offset %d: worst %.3f of the bound (%.3g at value %.6g)" % (seed, offset, q[k], err[k], got[k]))
        assert np.isfinite(got).all() and q[k] <= 1.0, (seed, offset, k, float(got[k]), float(ref[k]), float(err[k]), float(bound[k]))


def test_fill_sphere_points_against_numpy(env):
    """RA = 2pi u1 - pi, two roundings without contraction: bit for bit.  DEC = asin(2 u2 - 1) (the argument is exact) within
    GLIBC_ASIN_ULP + 4 ulp of the long double value."""
    pj, lib, dev = env
    assert np.finfo(np.longdouble).eps < 2e-19
    for seed, offset in GEN_CASES:
        t = torch.full((GEN_N, 2), NAN, dtype=torch.float64, device=dev)
        pj.fill_sphere_points_(t, seed, offset)
        got = t.cpu().numpy()
        u1, u2 = uniforms(seed, offset, GEN_N)
        assert bits_equal(got[:, 0], TWOPI * u1 - PI), (seed, offset)
        ref = np.arcsin((2.0 * u2 - 1.0).astype(np.longdouble))
        err = np.abs(got[:, 1].astype(np.longdouble) - ref).astype(np.float64)
        bound = (GLIBC_ASIN_ULP + DEVICE_EXTRA_ULP) * np.spacing(np.abs(ref.astype(np.float64)))
        q = err / bound
        k = int(np.argmax(q))
        print("fill_sphere seed %d offset %d: DEC worst %.3f of the bound" % (seed, offset, q[k]))
        assert np.isfinite(got).all() and bool((err <= bound).all()), (seed, offset, k, float(got[k, 1]), float(ref[k]), float(err[k]))


def test_fill_strips_equal_slices_above_the_grid_cap(env):
    """k_fill_random and k_fill_sphere take one element per work item: n = 2^28 + L elements pass the cap, so elements from
    2^28 on come from a second trip (k += 2^28).  The multi-rank benchmark relies on a strip generated with offset = its first
    index being the same slice of the whole: strips of 16 000 001 elements (odd: strip ends fall inside blocks) cover the
    whole buffer and are compared bit for bit, for both kinds and a non-zero base offset; three windows -- in the first trip,
    across the 2^28 boundary, at the tail -- are also compared with the NumPy reference directly."""
    pj, lib, dev = env
    n = CAP + L
    chunk = 16_000_001
    seed, base = 4242, (1 << 33) + 77
    windows = [(0, 200_000), (CAP - 100_000, 200_000), (n - 200_000, 200_000)]
    for kind in ("uniform", "normal"):
        big = torch.full((n,), NAN, dtype=torch.float64, device=dev)
        pj.fill_random_(big, seed, base, kind=kind)
        strip = torch.empty(chunk, dtype=torch.float64, device=dev)
        for lo in range(0, n, chunk):
            m = min(chunk, n - lo)
            pj.fill_random_(strip[:m].fill_(NAN), seed, base + lo, kind=kind)
            assert torch.equal(big[lo:lo + m], strip[:m]), (kind, lo, first_bad(big[lo:lo + m], strip[:m]))
        if kind == "uniform":
            for lo, m in windows:
                assert bits_equal(big[lo:lo + m].cpu().numpy(), uniforms(seed, base + lo, m)[0]), lo
        del big
    big = torch.full((n, 2), NAN, dtype=torch.float64, device=dev)
    pj.fill_sphere_points_(big, seed, base)
    strip = torch.empty((chunk, 2), dtype=torch.float64, device=dev)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        pj.fill_sphere_points_(strip[:m].fill_(NAN), seed, base + lo)
        assert torch.equal(big[lo:lo + m], strip[:m]), ("sphere", lo, first_bad(big[lo:lo + m], strip[:m]))
    for lo, m in windows:
        assert bits_equal(big[lo:lo + m, 0].cpu().numpy(), TWOPI * uniforms(seed, base + lo, m)[0] - PI), lo


# ================================================================================================
# 4. pxl_sample_build_pairs_*: the grid limits
# ================================================================================================

def test_build_pairs_grid_limit_falls_back_to_one_front(env, O):
    """2 columns, 65535 * 32 - 1 = 2 097 119 resident rows: tiles = ceil((rows + 1) / 32) = 65535, per = 8192 and per * fronts =
    65536 > 65535, so k_build_rowpairs runs with fronts = 1 and grid.y = 65535.  Sampling through that copy equals the oracle
    at points spread over the whole height (and the direct sampler)."""
    pj, lib, dev = env
    nx, ny = 2, 65535 * 32 - 1
    shape, wcs = car(pj, nx, ny)
    rng = np.random.default_rng(21)
    src = rng.normal(size=(ny, nx))
    m = pj.Enmap(to_dev(src, dev), wcs)
    pairs = pj.SamplePairs(m)
    npts = 400_000
    pix = np.stack([rng.uniform(0.5, nx + 0.5, npts), rng.uniform(0.5, ny + 0.5, npts)], axis=1)
    pix[:8, 1] = [1.0, 1.5, ny - 0.5, ny, ny - 31.5, ny - 32.5, 65535 * 32 - 33, 0.75]
    sky = O.pix2sky(wcs, pix, O.WRAP_NONE)
    exp = O.sample_bilinear(wcs, (nx, ny, 1), src[None], sky)
    d_sky = to_dev(sky, dev)
    got = pj.sample_bilinear(None, d_sky, pairs=pairs)
    assert np.array_equal(got.cpu().numpy(), exp) and not np.isnan(exp).any()
    assert torch.equal(pj.sample_bilinear(m, d_sky), got)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_build_pairs_refuses_more_row_tiles_than_the_grid_holds(env, dtype):
    """1 column, 65535 * 32 = 2 097 120 resident rows: tiles = ceil((rows + 1) / 32) = 65536 > 65535: PXL_EINVAL with the limit in
    the message, nothing written.  Source and pair buffer have the sizes the call describes (pxl_sample_pairs_elems).  One
    resident row fewer (tiles = 65535) is accepted."""
    pj, lib, dev = env
    ny = 65535 * 32
    shp = pj._lib.shape_arr((1, ny, 1))
    tdt = torch.float64 if dtype == "f64" else torch.float32
    nel = lib.pxl_sample_pairs_elems(shp, ny)
    assert nel > 0
    src = torch.ones(ny, dtype=tdt, device=dev)
    pairs = torch.full((nel,), NAN, dtype=tdt, device=dev)
    assert pairs.data_ptr() % 64 == 0
    fn = lib.pxl_sample_build_pairs_f64 if dtype == "f64" else lib.pxl_sample_build_pairs_f32
    assert fn(shp, P(src), ny, P(pairs), S(dev)) == EINVAL
    assert str(65535 * 32) in pj._lib.last_error(), pj._lib.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(pairs).all())
    assert fn(shp, P(src), ny - 1, P(pairs), S(dev)) == 0, pj._lib.last_error()
    assert not bool(torch.isnan(pairs).all())


# ================================================================================================
# the glibc figures (CPU only):  python tests/test_gpu_launch_paths.py
# ================================================================================================

def _glibc_figures():
    """Largest error of glibc's double precision log / sqrt / cos / asin (through Python's math module) on the formulas of
    k_fill_random and k_fill_sphere, against long double, on the inputs of the tests above."""
    assert np.finfo(np.longdouble).eps < 2e-19
    worst_bm = worst_as = 0.0
    for seed, offset in GEN_CASES:
        u1, u2 = uniforms(seed, offset, GEN_N)
        ref, r = boxmuller_ld(u1, u2)
        got = np.array([math.sqrt(-2.0 * math.log(1.0 - a)) * math.cos(TWOPI * b) for a, b in zip(u1.tolist(), u2.tolist())])
        e = np.abs(got.astype(np.longdouble) - ref).astype(np.float64) / np.spacing(r.astype(np.float64))
        worst_bm = max(worst_bm, float(e.max()))
        x = 2.0 * u2 - 1.0
        aref = np.arcsin(x.astype(np.longdouble))
        agot = np.array([math.asin(v) for v in x.tolist()])
        ok = aref != 0
        e = np.abs(agot.astype(np.longdouble) - aref).astype(np.float64)[ok] / np.spacing(np.abs(aref.astype(np.float64)))[ok]
        worst_as = max(worst_as, float(e.max()))
        print("seed %d offset %d: Box-Muller %.4f ulp(r), asin %.4f ulp (running maxima)" % (seed, offset, worst_bm, worst_as))
    print("GLIBC_BOXMULLER_ULP_R = %.3f   GLIBC_ASIN_ULP = %.3f" % (worst_bm, worst_as))


if __name__ == "__main__":
    _glibc_figures()
