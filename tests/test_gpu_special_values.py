"""The interpolating kernels on maps that hold NaN, +-Inf, -0.0, subnormal, huge and sentinel pixels (tests/special_values.py).

Bilinear paths: against the CPU oracle under SV.same -- NaN in the same positions, every other element equal as bits (sign of
zero, +-Inf, subnormals).  The oracle's own behaviour on these maps is pinned against its written definition, and the maps are
shown to reach enough outputs, in test_oracle_special_values.py.  Outputs are pre-filled with a sentinel (777.0).
Cubic path: the contract of DESIGN.md 4.9 / include/pixell_hip.h (a non-finite pixel is non-finite in every output whose 4 x 4
support holds it, its reach is REACH pixels along each axis, everything beyond is held to spline_ref.bound).
Distance transform: `== 0.0` decides what a zero pixel is (-0.0 is one; NaN, +-Inf and 5e-324 are not)."""
import ctypes as C
import math

import numpy as np
import pytest

import sdt_ref
import special_values as SV
import spline_ref as R
from conftest import DEG

torch = pytest.importorskip("torch")
from gpu_support import dev
pytestmark = pytest.mark.gpu

FILL = 777.0


def to_dev(a, dev, offset8=False):
    """the array on the device; offset8: 8 bytes past a 16-byte boundary (a view into a larger tensor)"""
    a = np.ascontiguousarray(a)
    if not offset8:
        return torch.from_numpy(a).to(dev)
    pad = 8 // a.dtype.itemsize
    owner = torch.empty(a.size + 2 * pad, dtype=torch.from_numpy(a).dtype, device=dev)
    assert owner.data_ptr() % 16 == 0
    view = owner[pad:pad + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8
    return view


def _oracle(O, wi, shape3, m, wo, so, **kw):
    if m.dtype == np.float32:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            return O.reproject_f32(wi, shape3, m, wo, so, **kw)
    return O.reproject(wi, shape3, m, wo, so, **kw)


def _run_plan(pj, dev, gin, gout, m, variant=0, offset8=False, **win):
    (si, wi), (so, wo) = gin, gout
    plan = pj.ReprojectPlan((si[0], si[1], m.shape[0]), wi, so, wo, device=dev, **win)
    plan.set_variant(variant)
    dst = torch.full(plan.dst_tensor_shape(), FILL, dtype=torch.from_numpy(m).dtype, device=dev)
    plan.execute(to_dev(m, dev, offset8), dst)
    got = dst.cpu().numpy()
    plan.close()
    return got


# ================================================================================================
# 3. bilinear CAR -> CAR
# ================================================================================================
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", SV.KINDS)
@pytest.mark.parametrize("name", SV.CAR_CASE_NAMES)
def test_reproject_every_kernel_form(pj, O, dev, name, kind, f32):
    """Every case of special_values.car_cases through the three kernel choices (0: LDS-DMA where the plan allows it, 1: direct
    gather, 2: register-staged), two components.  768-column periodic sources take k_reproject_dma in Float64 and Float32; the
    401-column box (odd nx) takes k_reproject_staged<.., false> under variant 0; wide_box_to_fullsky has the rewind jump inside
    a tile (the wave-uniform fallback: the source columns of the tile that holds the jump span more than a slot, asserted from
    the oracle's table); dec_flipped runs the swapped-weight blend with weights of exactly 0 and 1."""
    gin, gout, mode = SV.car_cases(pj)[name]
    (si, wi), (so, wo) = gin, gout
    if name == "wide_box_to_fullsky":
        xs, _ = O.reproject_tables(wi, si, wo, so)
        i0 = np.floor(xs)
        spans = [i0[c:c + 256].max() - i0[c:c + 256].min() for c in range(0, so[0], 256)]
        assert max(spans) > 5 * 128, "no 256-column tile of the output holds the rewind jump"      # PXL_MAXCH * 128: the largest slot
    m, _ = SV.case_map(O, kind, gin, gout, mode, seed=SV.case_seed(name), f32=f32, nc=2)
    exp = _oracle(O, wi, (si[0], si[1], 2), m, wo, so)
    for variant in (0, 1, 2):
        got = _run_plan(pj, dev, gin, gout, m, variant)
        SV.assert_same(got, exp, "%s %s variant %d" % (name, kind, variant))


@pytest.mark.parametrize("kind", SV.KINDS)
def test_reproject_unaligned_source(pj, O, dev, kind, monkeypatch):
    """A source 8 bytes off a 16-byte boundary: Float64 leaves the LDS-DMA kernel for k_reproject_staged<.., false>, Float32 for
    the gather kernel.  Then PXL_REPROJECT_PAIRS=1, off and on the boundary: k_reproject_staged<1, false> and <1, true>."""
    cases = SV.car_cases(pj)
    monkeypatch.setenv("PXL_REPROJECT_PAIRS", "1")
    for name in ("integer_shift", "half_pixel_shift", "dec_flipped"):
        gin, gout, mode = cases[name]
        (si, wi), (so, wo) = gin, gout
        m, _ = SV.case_map(O, kind, gin, gout, mode, seed=22)
        exp = _oracle(O, wi, (si[0], si[1], 1), m, wo, so)
        for offset8 in (True, False):
            SV.assert_same(_run_plan(pj, dev, gin, gout, m, 2, offset8=offset8), exp, "%s %s one pair per lane, offset8=%s" % (name, kind, offset8))
    monkeypatch.delenv("PXL_REPROJECT_PAIRS")
    for name in ("identity", "half_pixel_shift", "dec_flipped"):
        gin, gout, mode = cases[name]
        (si, wi), (so, wo) = gin, gout
        for f32 in (False, True):
            m, _ = SV.case_map(O, kind, gin, gout, mode, seed=21, f32=f32)
            exp = _oracle(O, wi, (si[0], si[1], 1), m, wo, so)
            for variant in (0, 2):
                SV.assert_same(_run_plan(pj, dev, gin, gout, m, variant, offset8=True), exp, "%s %s f32=%s variant %d" % (name, kind, f32, variant))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", SV.KINDS)
def test_reproject_every_tile_shape(pj, O, dev, kind, f32, monkeypatch):
    """The 3072 x 24 recipe of test_gpu_parity.test_reproject_every_tile_shape: PXL_REPROJECT_PAIRS 1, 2, 4 and a spread of RA
    scale factors, so that several chunk counts (NCH), partial last chunks and partial last tiles run.  Special values are placed
    on the seam pair, the first and last row and the source columns under output-tile boundaries, and sprinkled on top."""
    nx_in, ny_in = 3072, 24
    wcs_in = pj.CarClenshawCurtis((-360.0 / nx_in, 2.0), (nx_in / 2 + 0.5, 12.0), (0.3, 0.0))
    gin = ((nx_in, ny_in), wcs_in)
    rng = np.random.default_rng(321)
    for pairs in (1, 2, 4):
        monkeypatch.setenv("PXL_REPROJECT_PAIRS", str(pairs))
        for sx in (0.2, 0.7, 1.0, 1.45, 2.4, 3.4, 4.9):
            nxo = max(64, int(round(nx_in / sx)) & ~1)
            dy = 12.0 if sx == 1.0 else 12.3                          # sx = 1: integer offsets in both axes
            sc = 1.0 if sx == 1.0 else rng.uniform(0.9, 1.1)
            wcs_out = pj.CarClenshawCurtis((-360.0 / nxo, 2.0 * sc), (nxo / 2 + (0.5 if sx == 1.0 else 0.25), dy), (0.3, 0.0))
            gout = ((nxo, 20), wcs_out)
            m, mask = SV.case_map(O, kind, gin, gout, "placed", seed=pairs, f32=f32, nc=2)
            if kind != "neg_zero_all":
                extra, emask = SV.special_map(kind, gin[0], nc=2, seed=pairs + 10, f32=f32, mode="sprinkled")
                m = np.where(emask[None], extra, m)
            exp = _oracle(O, wcs_in, (nx_in, ny_in, 2), m, wcs_out, gout[0])
            if kind in SV.NONFINITE:
                bad = ~np.isfinite(exp)
                assert bad.mean() >= 0.05 and (~bad).mean() >= 0.5, (kind, pairs, sx, float(bad.mean()))
            SV.assert_same(_run_plan(pj, dev, gin, gout, m), exp, "%s pairs %d sx %g" % (kind, pairs, sx))


@pytest.mark.parametrize("pairs", [1, 2, 4])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", SV.KINDS)
def test_reproject_direct_tap_fallback(pj, O, dev, kind, f32, pairs, monkeypatch):
    """The wave-uniform direct-tap fallback of the two tile kernels at every lane width and in both storage types.  A 1432 x 24
    box of 0.25-degree pixels (not periodic; its pixel period is 1440 columns) goes onto a 1440-column ring of the same
    resolution whose RA centre lies 100 degrees away, so the box's rewind jump falls at output column 400: inside a tile of every
    width, 128 * pairs columns in Float64 and 256 * pairs in Float32.  The tile that holds the jump then spans about 1440 source
    columns, more than the largest slot of either storage type (640 doubles, 1280 floats), which is asserted from the oracle's
    table for the width under test before the device runs.  Variant 0 is k_reproject_dma<T, pairs, .>; variant 2, in Float64 at
    lane widths 1 and 2, is k_reproject_staged<pairs, true>."""
    nx_in, ny_in, nxo, nyo = 1432, 24, 1440, 20
    wcs_in = pj.CarClenshawCurtis((-0.25, 0.25), (nx_in / 2 + 0.5, 12.0), (0.0, 0.0))
    wcs_out = pj.CarClenshawCurtis((-360.0 / nxo, 0.27), (nxo / 2 + 0.25, 10.3), (100.0, 0.0))
    gin, gout = ((nx_in, ny_in), wcs_in), ((nxo, nyo), wcs_out)
    assert not O.is_periodic(wcs_in, nx_in)
    xs, _ = O.reproject_tables(wcs_in, gin[0], wcs_out, gout[0])
    i0 = np.floor(xs)
    width, slot = (256 * pairs, 5 * 256) if f32 else (128 * pairs, 5 * 128)          # PXL_MAXCH accesses: the largest slot
    spans = [i0[c:c + width].max() - i0[c:c + width].min() for c in range(0, nxo, width)]
    assert max(spans) > slot, "no %d-column tile of the output spans more than a slot of %d source columns" % (width, slot)
    monkeypatch.setenv("PXL_REPROJECT_PAIRS", str(pairs))
    m, _ = SV.case_map(O, kind, gin, gout, "sprinkled", seed=40 + pairs, f32=f32, nc=2)
    exp = _oracle(O, wcs_in, (nx_in, ny_in, 2), m, wcs_out, gout[0])
    for variant in ((0,) if f32 or pairs == 4 else (0, 2)):
        SV.assert_same(_run_plan(pj, dev, gin, gout, m, variant), exp, "%s f32=%s pairs %d variant %d" % (kind, f32, pairs, variant))


@pytest.mark.parametrize("kind", SV.KINDS)
def test_reproject_row_windows(pj, O, dev, kind):
    """src_rows / dst_rows windows with special values on the first and last resident row, execute_rows in two pieces, and a
    window two rows short on each side whose missing rows are special in the full map: they must read as the value 0.0."""
    cases = SV.car_cases(pj)
    for name in ("integer_shift", "half_pixel_shift", "dec_flipped"):
        gin, gout, mode = cases[name]
        (si, wi), (so, wo) = gin, gout
        lo, n = 120, 90
        s_lo, s_hi = O.reproject_src_rows(wi, si, wo, so, lo, n)
        for f32 in (False, True):
            m, _ = SV.case_map(O, kind, gin, gout, mode, seed=7, f32=f32, rows=(s_lo, s_lo + 1, s_hi - 2, s_hi - 1))
            for cut in (0, 2):
                a, b = s_lo + cut, s_hi - cut
                kw = dict(src_row0=a, src_nrows=b - a, dst_row0=lo, dst_nrows=n)
                exp = _oracle(O, wi, (si[0], si[1], 1), m[:, a:b], wo, so, **kw)
                for variant in (0, 1, 2):
                    got = _run_plan(pj, dev, gin, gout, m[:, a:b], variant, src_rows=(a, b - a), dst_rows=(lo, n))
                    SV.assert_same(got, exp, "%s %s f32=%s cut %d variant %d" % (name, kind, f32, cut, variant))
                plan = pj.ReprojectPlan((si[0], si[1], 1), wi, so, wo, src_rows=(a, b - a), dst_rows=(lo, n), device=dev)
                dst = torch.full(plan.dst_tensor_shape(), FILL, dtype=torch.float32 if f32 else torch.float64, device=dev)
                s = to_dev(m[:, a:b], dev)
                plan.build_tables()
                plan.execute_rows(s, dst, 37, n - 37)
                plan.execute_rows(s, dst, 0, 37)
                SV.assert_same(dst.cpu().numpy(), exp, "%s %s f32=%s cut %d in two pieces" % (name, kind, f32, cut))
                plan.close()


# ================================================================================================
# 4. scattered bilinear sampling
# ================================================================================================
def _sample_oracle(O, wi, shape3, m, sky, **kw):
    if m.dtype == np.float32:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            return O.sample_bilinear_f32(wi, shape3, m, sky, **kw)
    return O.sample_bilinear(wi, shape3, m, sky, **kw)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", SV.KINDS)
def test_sample_direct_and_pairs(pj, O, dev, kind, f32):
    """k_sample_bilinear and k_build_rowpairs + k_sample_pairs against the oracle and against each other.  Points: uniform on
    the sphere, exact centres of special pixels and of their eight neighbours, the last half pixel beyond every edge, seam cells.
    Point 0 has a NaN RA: the first 16 bytes of `sky`, where the direct kernel aims the loads of points that are not `wide`,
    then read as NaN map elements (Float64: the first element; Float32: the first two).  A point cannot both have that bit
    pattern and sample a pixel -- a NaN coordinate samples nothing -- so the second request of the issue for point 0 (that it
    sample a special pixel itself) goes to point 1, the exact centre of pixel (1, 1).  Pixel (1, 1) is special in every case (a
    corner): entry 0 of every pair plane, which the pair kernel loads for off-map entries.  Row windows carry special values on
    their first and last resident row.  Sprinkled maps: at least 5 % of the on-map points give a non-finite value and at
    least half a finite one (non-finite kinds)."""
    cases = SV.car_cases(pj)
    rng = np.random.default_rng(11)
    for name, mode in (("identity", "placed"), ("half_pixel_shift", "sprinkled"), ("sub_box_onto_full_sky", "placed"),
                       ("wide_box_to_fullsky", "placed")):
        (si, wi) = cases[name][0]
        m, mask = SV.special_map(kind, si, nc=2, seed=3, f32=f32, mode=mode, rows=(100, 149))
        if kind != "neg_zero_all":
            m[:, 0, 0] = SV._values(kind, 1, rng, f32)[0]              # pixel (1, 1) holds the kind's value in both modes
            mask[0, 0] = True
        sky = SV.sky_points(rng, si, wi, mask)
        corner = [(wi.crval[0] + (1.0 - wi.crpix[0]) * wi.cdelt[0]) * wi.unit, (wi.crval[1] + (1.0 - wi.crpix[1]) * wi.cdelt[1]) * wi.unit]
        sky = np.concatenate([[[np.nan, 0.3], corner], sky])
        exp = _sample_oracle(O, wi, (si[0], si[1], 2), m, sky)
        if mode == "sprinkled" and kind in SV.NONFINITE:
            on_map = _sample_oracle(O, wi, (si[0], si[1], 1), np.ones((1, si[1], si[0])), sky)[0] > 0.999
            bad = ~np.isfinite(exp[:, on_map])
            assert bad.mean() >= 0.05 and (~bad).mean() >= 0.5, (name, kind, float(bad.mean()))
        d_sky = to_dev(sky, dev)
        em = pj.Enmap(to_dev(m, dev), wi)
        direct = pj.sample_bilinear(em, d_sky).cpu().numpy()
        SV.assert_same(direct, exp, "direct %s %s" % (name, kind))
        paired = pj.sample_bilinear(None, d_sky, pairs=pj.SamplePairs(em)).cpu().numpy()
        SV.assert_same(paired, exp, "pairs %s %s" % (name, kind))
        SV.assert_same(paired, direct, "pairs against direct %s %s" % (name, kind))
        # row windows: cells that straddle the window edges, a one-row window, an empty one
        for r0, nr in ((100, 50), (si[1] - 1, 1), (40, 0)):
            sub = np.ascontiguousarray(m[:, r0:r0 + nr])
            expw = _sample_oracle(O, wi, (si[0], si[1], 2), sub, sky, src_row0=r0, src_nrows=nr)
            ew = pj.Enmap(to_dev(sub, dev), wi)
            got = pj.sample_bilinear(ew, d_sky, src_rows=(r0, nr), full_shape=(si[0], si[1], 2)).cpu().numpy()
            SV.assert_same(got, expw, "direct window %s %s %s" % (name, kind, (r0, nr)))
            if nr > 0:
                sp = pj.SamplePairs(ew, src_rows=(r0, nr), full_shape=(si[0], si[1], 2))
                SV.assert_same(pj.sample_bilinear(None, d_sky, pairs=sp).cpu().numpy(), expw, "pairs window %s %s %s" % (name, kind, (r0, nr)))


@pytest.mark.parametrize("kind", SV.KINDS)
def test_sample_one_pixel_maps(pj, O, dev, kind):
    """1 x 1 maps, periodic and not, whose only pixel is special (test_gpu_parity.test_sample_degenerate_windows with values):
    Float64 and Float32, the direct kernel and the pair kernel."""
    rng = np.random.default_rng(5)
    n = 2000
    sky = np.stack([2 * math.pi * rng.random(n) - math.pi, np.arcsin(2 * rng.random(n) - 1)], axis=1)
    near = np.stack([0.02 * (rng.random(n) - 0.5), 0.02 * (rng.random(n) - 0.5)], axis=1)
    both = np.concatenate([[[0.0, 0.0]], near, sky])
    for periodic in (True, False):
        w1 = pj.CarClenshawCurtis((-360.0, 180.0), (1.0, 1.0), (0.0, 0.0)) if periodic else \
            pj.CarClenshawCurtis((-1.0, 1.0), (1.0, 1.0), (0.0, 0.0))
        for f32 in (False, True):
            v1 = SV._values("neg_zero" if kind == "neg_zero_all" else kind, 1, rng, f32)[0]
            src = np.array([[[v1]]], dtype=np.float32 if f32 else np.float64)
            exp = _sample_oracle(O, w1, (1, 1, 1), src, both)
            em = pj.Enmap(to_dev(src, dev)[0], w1)
            got = pj.sample_bilinear(em, to_dev(both, dev)).cpu().numpy()
            SV.assert_same(got, exp, "1 x 1 %s periodic=%s f32=%s direct" % (kind, periodic, f32))
            got = pj.sample_bilinear(None, to_dev(both, dev), pairs=pj.SamplePairs(em)).cpu().numpy()
            SV.assert_same(got, exp, "1 x 1 %s periodic=%s f32=%s pairs" % (kind, periodic, f32))


# ================================================================================================
# 5. CAR <-> Gnomonic
# ================================================================================================
def _generic_compare(got, exp, scale, tag):
    """NaN in the same positions; +-Inf and zeros (with their sign) exactly; finite elements within 1e-9 of the oracle, the
    bound of test_gpu_interpolated.py, unchanged for every output whose taps are ordinary data.  An output whose own 2 x 2 cell
    holds a finite special value M (sentinel, huge) is allowed 1e-9 max(1, |M|): the two sides differ by rounding in the
    coordinates, which moves a value by that shift times the differences of its taps.  `scale` (per output element) comes from
    _special_scale: 0 for ordinary cells, at least the largest |special tap| of the cell otherwise."""
    assert np.array_equal(np.isnan(got), np.isnan(exp)), (tag, "NaN positions", int((np.isnan(got) != np.isnan(exp)).sum()))
    inf = np.isinf(exp)
    assert np.array_equal(got[inf], exp[inf]) and np.array_equal(np.isinf(got), inf), (tag, "Inf")
    zero = exp == 0
    assert np.array_equal(got[zero].view(np.int64), exp[zero].view(np.int64)), (tag, "zeros and their sign")
    fin = np.isfinite(exp)
    with np.errstate(over="ignore"):
        err = np.abs(got[fin] - exp[fin])                  # an overflowing difference is inf and fails
    tol = 1e-9 * np.maximum(1.0, scale[fin])
    bad = err > tol
    assert not bad.any(), (tag, int(bad.sum()), float(err[bad].max()), float(tol[bad].min()))
    assert (scale[fin] == 0).mean() > 0.5, (tag, "most outputs must keep the plain 1e-9 bound")


def _special_scale(O, m, mask, gin, pin, gout, pout):
    """Per output element: 0 where none of the four taps is a special pixel, otherwise a number that is at least the largest
    |finite special tap| of the cell.  The magnitudes of the finite special pixels (0 elsewhere) are spread over each 3 x 3
    neighbourhood (columns wrap) and reprojected by the oracle: every tap of a cell then carries the maximum over a window that
    holds the whole cell, and a weighted mean of four such numbers is no smaller than that maximum.  Outputs within a pixel of
    a special one may get a non-zero scale without having a special tap; that only applies the looser bound to a few more."""
    (si, wi), (so, wo) = gin, gout
    b = np.where(mask[None] & np.isfinite(m), np.abs(m), 0.0)
    d = b.copy()
    for dy in (-1, 0, 1):
        s = b if dy == 0 else np.concatenate([b[:, 1:], b[:, -1:]], axis=1) if dy == 1 else np.concatenate([b[:, :1], b[:, :-1]], axis=1)
        for dx in (-1, 0, 1):
            d = np.maximum(d, np.roll(s, dx, axis=2))
    with np.errstate(over="ignore"):
        out = O.reproject_generic(wi, pin, (si[0], si[1], 1), d, wo, pout, so)
    return np.where(np.isfinite(out), out, np.inf)


@pytest.mark.parametrize("kind", SV.KINDS)
def test_generic_reprojection(pj, O, dev, kind, monkeypatch):
    """CAR -> TAN (a patch across the RA seam) and TAN -> CAR onto the full sky (half the sky is not visible from the source
    plane and reads as 0 whatever the map holds at the mirror-image position the plane formula gives): one-shot (lattice, tiled
    and exact-tile kernels), one-shot with PXL_GENERIC_EXACT=1 (k_reproject_generic, every pixel evaluated on its own) and
    through a GenericReprojectPlan; placed and sprinkled.  Each sprinkled map must reach at least 5 % of the visible outputs
    and leave at least half of them finite (non-finite kinds)."""
    fs = pj.fullsky_geometry(2 * math.pi / 2160)                       # 10' full sky
    tan_out = ((384, 256), pj.Gnomonic((-10.0 / 60, 10.0 / 60), (192.5, 128.5), (179.0, 10.0)))
    tan_src = ((400, 300), pj.Gnomonic((-10.0 / 60, 10.0 / 60), (200.5, 150.5), (20.0, -15.0)))
    fs_out = pj.fullsky_geometry(2 * math.pi / 720)
    for name, gin, gout in (("car_to_tan", fs, tan_out), ("tan_to_car", tan_src, fs_out)):
        (si, wi), (so, wo) = gin, gout
        pin, pout = int(isinstance(wi, pj.Gnomonic)), int(isinstance(wo, pj.Gnomonic))
        for mode in ("placed", "sprinkled"):
            m, mask = SV.special_map(kind, si, nc=1, seed=5, mode=mode)
            exp = O.reproject_generic(wi, pin, (si[0], si[1], 1), m, wo, pout, so)
            if kind == "neg_zero_all":
                scale = np.zeros(exp.shape)
            else:
                scale = _special_scale(O, m, mask, gin, pin, gout, pout)
            if mode == "sprinkled" and kind in SV.NONFINITE:
                seen = O.reproject_generic(wi, pin, (si[0], si[1], 1), np.ones(m.shape), wo, pout, so) > 0.5
                bad = ~np.isfinite(exp[seen])
                assert bad.mean() >= 0.05 and (~bad).mean() >= 0.5, (name, kind, float(bad.mean()))
            em = pj.Enmap(to_dev(m, dev), wi)
            got = pj.reproject(em, so, wo).data.cpu().numpy()
            _generic_compare(got, exp, scale, "%s %s %s one-shot" % (name, kind, mode))
            monkeypatch.setenv("PXL_GENERIC_EXACT", "1")
            per_pixel = pj.reproject(em, so, wo).data.cpu().numpy()
            monkeypatch.delenv("PXL_GENERIC_EXACT")
            _generic_compare(per_pixel, exp, scale, "%s %s %s per pixel" % (name, kind, mode))
            plan = pj.GenericReprojectPlan(si, wi, so, wo, device=dev)
            out = pj.Enmap(torch.full((1, so[1], so[0]), FILL, dtype=torch.float64, device=dev), wo)
            pj.reproject(em, so, wo, out=out, plan=plan)
            SV.assert_same(out.data.cpu().numpy(), got, "%s %s %s plan against one-shot" % (name, kind, mode))
            plan.close()


# ================================================================================================
# 6. cubic B-spline
# ================================================================================================
# Reach of a non-finite pixel along one axis.  k_spline_prefilter gives each lane PXL_SPL_SUB = 16 consecutive outputs, which it
# computes from the inputs PXL_SPL_WARM = 32 positions before its first output to 32 after its last; a
# non-finite input anywhere in that span of 80 makes the causal recursion non-finite from there on and the anti-causal sweep,
# which starts from the far end, non-finite over all of it.  An output at position o of a lane whose outputs start at s
# (s <= o <= s + 15) therefore sees inputs s - 32 .. s + 47: a pixel at t reaches o iff |o - t| <= 47 at most.  Mirror images
# lie farther from o than the pixel itself (|o - (2 - t)| = o + t - 2 >= |o - t|), cyclic images are at the cyclic distance.
# An evaluated value is reached where one of its 4 x 4 taps is (the tests dilate the reach through the taps themselves).
WARM, SUB = 32, 16
REACH = WARM + SUB - 1


def _reach_mask(bad, periodic, reach):
    """pixels within `reach` columns and `reach` rows of a non-finite pixel (cyclic distance along a periodic RA axis)"""
    ny, nx = bad.shape
    cols = bad.copy()
    for d in range(1, reach + 1):
        if periodic:
            cols |= np.roll(bad, d, axis=1) | np.roll(bad, -d, axis=1)
        else:
            cols[:, d:] |= bad[:, :-d]
            cols[:, :-d] |= bad[:, d:]
    out = cols.copy()
    for d in range(1, reach + 1):
        out[d:] |= cols[:-d]
        out[:-d] |= cols[d:]
    return out


def _spots(shape):
    """special pixels next to a segment boundary (256) and a line-group boundary (16) of both prefilter passes, on the map edge
    (mirror rule / seam) and in the interior; 0-based (row, column)"""
    nx, ny = shape
    s = [(0, 0), (ny - 1, nx - 1), (ny // 2, 0), (ny // 2 + 3, nx - 1), (15, 255), (16, 256), (ny // 3, nx // 2)]
    if ny > 300:
        s += [(255, 15), (256, 16)]
    return [(j, i) for j, i in s if j < ny and i < nx]


@pytest.mark.parametrize("kind", SV.NONFINITE)
@pytest.mark.parametrize("geom", ["cc_1024x513", "box_600x300"])
def test_cubic_nonfinite_contract(pj, O, dev, geom, kind):
    """A handful of non-finite pixels: the coefficient at each is non-finite; every coefficient outside the reach is finite and
    held to spline_ref.bound against the yardstick of the map with those pixels replaced by 0.0 (any finite replacement changes
    a coefficient REACH pixels away by |z|^47 = 1e-27 of its size, far below the bound of 24 eps); the same for reproject and
    sample with the evaluation's reach; outputs whose 4 x 4 support holds a non-finite pixel are non-finite; out-of-domain
    outputs are exactly +0.0; two calls agree."""
    if geom == "cc_1024x513":
        shape, wcs = R.geometries(pj)["cc_1024x513"]
    else:
        shape, wcs = pj.geometry([[60 * DEG, -60 * DEG], [-30 * DEG, 30 * DEG]], 0.2 * DEG)
        assert shape == (600, 300)
    nx, ny = shape
    per = pj.is_periodic(wcs, nx)
    rng = np.random.default_rng(len(geom))
    m = rng.normal(size=(ny, nx))
    bad = np.zeros((ny, nx), bool)
    for j, i in _spots(shape):
        bad[j, i] = True
    vals = SV._values(kind, int(bad.sum()), rng, False)
    m[bad] = vals
    if kind == "mixed_inf":
        m[ny // 3, nx // 2 + 1] = -np.inf                          # adjacent +Inf and -Inf
        bad[ny // 3, nx // 2 + 1] = True
    clean = np.where(bad, 0.0, m)
    em = pj.Enmap(to_dev(m, dev), wcs)
    # -- coefficients
    got = pj.spline_prefilter(em).data.cpu().numpy()
    assert SV.same(got, pj.spline_prefilter(em).data.cpu().numpy())[0], "two calls differ"
    assert not np.isfinite(got[bad]).any(), "the coefficient at a non-finite pixel must be non-finite"
    near = _reach_mask(bad, per, REACH)
    assert np.isfinite(got[~near]).all(), "a coefficient outside the reach is not finite"
    assert (~near).mean() > 0.3
    ref = R.prefilter(clean, per)
    r = float(np.abs(got[~near] - ref[~near]).max() / R.bound(clean)[0])
    print("%s %s: coefficients outside the reach, worst error / bound = %.3g" % (geom, kind, r))
    assert r <= 1.0
    # -- reprojection: a refinement (rows reused), and a coarser DEC-flipped grid (the row window moves backwards)
    fine = ((2 * nx, 2 * ny - 1), R.shifted(wcs, 0.0, 0.0, 2))
    flip = ((nx // 3, ny // 3), type(wcs)((3.3 * wcs.cdelt[0], -3.1 * wcs.cdelt[1]), (nx / 6 + 0.3, ny / 6 + 0.2), wcs.crval))
    wide = None if per else ((nx + 80, ny + 60), R.shifted(wcs, -40.25, -30.25, 1))     # the box inside a larger grid
    for tag, (so, wo) in [("refine", fine), ("coarse flipped", flip)] + ([] if per else [("margin", wide)]):
        xs, ys = O.reproject_tables(wcs, shape, wo, so)
        out = pj.reproject(em, so, wo, order=3).data.cpu().numpy()
        assert SV.same(out, pj.reproject(em, so, wo, order=3).data.cpu().numpy())[0], tag + ": two calls differ"
        okx = np.ones(len(xs), bool) if per else R.in_domain(xs, nx)
        oky = R.in_domain(ys, ny)
        inside = oky[:, None] & okx[None, :]
        z = out[~inside]
        assert np.array_equal(z.view(np.int64), np.zeros(z.shape, np.int64)), tag + ": out-of-domain pixels must be +0.0"
        if tag == "margin":
            assert (~inside).any()
        i0 = np.where(okx, np.floor(xs), 1).astype(np.int64)
        j0 = np.where(oky, np.floor(ys), 1).astype(np.int64)

        def touched(msk):
            t = np.zeros((len(ys), len(xs)), bool)
            for b in range(4):
                rows = R.fold(j0 - 1 + b, ny, False) - 1
                for a in range(4):
                    cols = R.fold(i0 - 1 + a, nx, per) - 1
                    t |= msk[np.ix_(rows, cols)]
            return t & inside
        support = touched(bad)
        assert support.any() and not np.isfinite(out[support]).any(), tag + ": a finite value from a non-finite pixel"
        far = inside & ~touched(near)
        assert far.mean() > 0.1, (tag, far.mean())
        assert np.isfinite(out[far]).all(), tag + ": not finite outside the reach"
        refo = R.evaluate(ref, xs, ys, per)
        r = float(np.abs(out[far] - refo[far]).max() / R.bound(clean)[0])
        print("%s %s reproject %s: outside the reach, worst error / bound = %.3g" % (geom, kind, tag, r))
        assert r <= 1.0, tag
    # -- scattered points: uniform, and round the non-finite pixels
    sky = R.sphere_points(20000, 7)
    jj, ii = np.nonzero(bad)
    ring = np.concatenate([np.stack([ii + 1.0 + dx, jj + 1.0 + dy], axis=1) for dx in (-1.5, -1, 0, 0.25, 1, 2.0) for dy in (-2.0, -1, 0, 0.5, 1, 1.5)])
    a = (wcs.crval[0] + (ring[:, 0] - wcs.crpix[0]) * wcs.cdelt[0]) * wcs.unit
    d = (wcs.crval[1] + (ring[:, 1] - wcs.crpix[1]) * wcs.cdelt[1]) * wcs.unit
    sky = np.concatenate([sky, np.stack([a, d], axis=1)])
    pix = O.sky2pix(wcs, shape, sky, safe=True)
    x, y = pix[:, 0], pix[:, 1]
    out = pj.sample(em, to_dev(sky, dev), order=3).cpu().numpy()[0]
    assert SV.same(out, pj.sample(em, to_dev(sky, dev), order=3).cpu().numpy()[0])[0]
    inside = R.in_domain(y, ny) & (np.ones(len(x), bool) if per else R.in_domain(x, nx))
    assert np.array_equal(out[~inside].view(np.int64), np.zeros(int((~inside).sum()), np.int64))
    i0 = np.where(inside, np.floor(x), 1).astype(np.int64)
    j0 = np.where(inside, np.floor(y), 1).astype(np.int64)

    def touched_pts(msk):
        t = np.zeros(len(x), bool)
        for b in range(4):
            rows = R.fold(j0 - 1 + b, ny, False) - 1
            for a_ in range(4):
                t |= msk[rows, R.fold(i0 - 1 + a_, nx, per) - 1]
        return t & inside
    support = touched_pts(bad)
    assert support.sum() >= len(jj) and not np.isfinite(out[support]).any()
    far = inside & ~touched_pts(near)
    assert far.sum() > 1000 and np.isfinite(out[far]).all()
    refp = R.evaluate_points(ref, x, y, per)
    r = float(np.abs(out[far] - refp[far]).max() / R.bound(clean)[0])
    print("%s %s sample: outside the reach, worst error / bound = %.3g" % (geom, kind, r))
    assert r <= 1.0


@pytest.mark.parametrize("kind", ["neg_zero_all", "neg_zero", "subnormal", "huge", "sentinel"])
def test_cubic_finite_kinds(pj, O, dev, kind):
    """Finite special values go through the ordinary check against the yardstick.  `huge` is scaled (1.7e308 / 64) so that the
    yardstick itself stays finite (the coefficients of an isolated spike are up to ~3x the spike), which is asserted."""
    shape, wcs = R.geometries(pj)["cc_1024x513"]
    per = True
    for mode in ("placed", "sprinkled"):
        m, _ = SV.special_map(kind, shape, nc=1, seed=9, mode=mode)
        m = m[0]
        if kind == "huge":
            m = np.where(np.abs(m) > 1e300, m / 64, m)
        ref = R.prefilter(m, per)
        assert np.isfinite(ref).all()
        em = pj.Enmap(to_dev(m, dev), wcs)
        got = pj.spline_prefilter(em).data.cpu().numpy()
        r = R.worst_ratio(got, ref, m) if np.abs(m).max() > 0 else float(np.abs(got).max())
        print("cubic %s %s: prefilter worst error / bound = %.3g" % (kind, mode, r))
        assert r <= (1.0 if np.abs(m).max() > 0 else 0.0)
        so, wo = (2048, 1025), R.shifted(wcs, 0.0, 0.0, 2)
        xs, ys = O.reproject_tables(wcs, shape, wo, so)
        refo = R.evaluate(ref, xs, ys, per)
        assert np.isfinite(refo).all()
        out = pj.reproject(em, so, wo, order=3).data.cpu().numpy()
        r = R.worst_ratio(out, refo, m) if np.abs(m).max() > 0 else float(np.abs(out).max())
        print("cubic %s %s: reproject worst error / bound = %.3g" % (kind, mode, r))
        assert r <= (1.0 if np.abs(m).max() > 0 else 0.0)
        sky = R.sphere_points(20000, 8)
        pix = O.sky2pix(wcs, shape, sky, safe=True)
        refp = R.evaluate_points(ref, pix[:, 0], pix[:, 1], per)
        assert np.isfinite(refp).all()
        pts = pj.sample(em, to_dev(sky, dev), order=3).cpu().numpy()[0]
        r = R.worst_ratio(pts, refp, m) if np.abs(m).max() > 0 else float(np.abs(pts).max())
        print("cubic %s %s: sample worst error / bound = %.3g" % (kind, mode, r))
        assert r <= (1.0 if np.abs(m).max() > 0 else 0.0)


# ================================================================================================
# 7. distance transform
# ================================================================================================
@pytest.mark.parametrize("kind", ["nan", "+inf", "-inf", "mixed_inf", "subnormal", "huge", "sentinel"])
def test_distance_transform_nonzero_values(pj, dev, kind):
    """A mask whose non-zero pixels are all of one special kind (5e-324 and 2e-308 among the subnormals: not zero), its zeros
    written as +0.0 and -0.0 at random; one row whose only zero is -0.0.  Per-pixel bound of sdt_ref; zero pixels exactly +0.0."""
    shape, wcs = pj.fullsky_geometry(2 * DEG)
    nx, ny = shape
    rng = np.random.default_rng(31)
    m = SV._values(kind, nx * ny, rng, False).reshape(ny, nx)
    assert (m != 0).all()
    zeros = rng.random((ny, nx)) < 0.01
    zeros[ny // 2] = False
    zeros[ny // 2 + 1] = False
    zeros[ny // 2 - 1] = False
    zeros[ny // 2, 17] = True                                          # the only zero of three rows, written as -0.0
    m[zeros] = np.where(rng.random(int(zeros.sum())) < 0.5, -0.0, 0.0)
    m[ny // 2, 17] = -0.0
    got = pj.distance_transform(pj.ExactSeqSDT(), pj.Enmap(to_dev(m, dev), wcs)).data.cpu().numpy()
    ref = sdt_ref.distance_transform(m, wcs)
    zero = m == 0
    assert np.array_equal(zero, zeros)
    assert np.array_equal(got[zero].view(np.int64), np.zeros(int(zero.sum()), np.int64)), "zero pixels must be exactly +0.0"
    r = sdt_ref.worst_ratio(got, ref)
    print("distance transform %s: worst error / bound = %.3g" % (kind, r))
    assert r <= 1.0


def test_distance_transform_subnormals_are_not_zero(pj, dev):
    """A map whose smallest values are subnormal (5e-324, 2e-308, negative ones too) and which has no zero: ValueError from
    Python, +Inf everywhere from the C entry."""
    shape, wcs = pj.fullsky_geometry(4 * DEG)
    nx, ny = shape
    rng = np.random.default_rng(32)
    m = rng.normal(size=(ny, nx))
    tiny = rng.random((ny, nx)) < 0.2
    m[tiny] = SV._values("subnormal", int(tiny.sum()), rng, False)
    assert (m != 0).all() and (np.abs(m) < 2.3e-308).any()
    d_m = to_dev(m, dev)
    with pytest.raises(ValueError):
        pj.distance_transform(pj.ExactSeqSDT(), pj.Enmap(d_m, wcs))
    out = torch.full((ny, nx), FILL, dtype=torch.float64, device=dev)
    w = wcs.to_struct()
    rc = pj.load_library().pxl_distance_transform_car_f64(C.byref(w), pj._lib.shape_arr(shape), C.c_void_p(d_m.data_ptr()),
                                                          C.c_void_p(out.data_ptr()),
                                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, pj._lib.last_error()
    assert bool(torch.isinf(out).all()) and bool((out > 0).all())
