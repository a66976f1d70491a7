"""The oracle's bilinear entries on NaN, +-Inf, -0.0, subnormal, huge and sentinel pixels, against the written definition R1
(oracle/pixell_oracle.c) restated in plain numpy (tests/special_values.py): off-map and off-window taps are the VALUE 0.0 and
are then multiplied by their weight, so an in-map NaN with weight 0 gives NaN while an off-map tap never does.  The device is
compared with the oracle on the same maps in test_gpu_special_values.py; this file is what makes the oracle a judge there, and
it holds the non-vacuity conditions of those maps (checked with the oracle alone)."""
import math

import numpy as np
import pytest

import special_values as SV

DEG = math.pi / 180


@pytest.mark.parametrize("kind", SV.KINDS)
def test_reproject_matches_written_definition(pj, O, kind):
    """O.reproject and O.reproject_f32 against R1 in numpy on every case of special_values.car_cases, every kind."""
    for name, (gin, gout, mode) in SV.car_cases(pj).items():
        (si, wi), (so, wo) = gin, gout
        for f32 in (False, True):
            m, mask = SV.case_map(O, kind, gin, gout, mode, seed=SV.case_seed(name), f32=f32)
            if f32:
                got = O.reproject_f32(wi, si, m, wo, so)
                exp = SV.to_f32(SV.r1_reproject(O, wi, si, m.astype(np.float64), wo, so))
            else:
                with np.errstate(all="ignore"):
                    got = O.reproject(wi, si, m, wo, so)
                exp = SV.r1_reproject(O, wi, si, m, wo, so)
            SV.assert_same(got, exp, "%s %s f32=%s" % (name, kind, f32))


@pytest.mark.parametrize("kind", SV.KINDS)
def test_reproject_windows_match_written_definition(pj, O, kind):
    """Row windows: special values on the first and last resident row; and special rows just outside the window, present in the
    full map and absent from the resident buffer, which must not appear (the taps there are the value 0.0)."""
    cases = SV.car_cases(pj)
    for name in ("integer_shift", "half_pixel_shift"):
        gin, gout, mode = cases[name]
        (si, wi), (so, wo) = gin, gout
        lo, n = 120, 90
        s_lo, s_hi = O.reproject_src_rows(wi, si, wo, so, lo, n)
        m, mask = SV.case_map(O, kind, gin, gout, mode, seed=7, rows=(s_lo, s_hi - 1))
        full = O.reproject(wi, si, m, wo, so)
        win = O.reproject(wi, si, m[:, s_lo:s_hi], wo, so, src_row0=s_lo, src_nrows=s_hi - s_lo, dst_row0=lo, dst_nrows=n)
        SV.assert_same(win, full[:, lo:lo + n], "%s %s: window against the full map" % (name, kind))
        SV.assert_same(win, SV.r1_reproject(O, wi, si, m[:, s_lo:s_hi], wo, so, src_row0=s_lo, dst_row0=lo, dst_nrows=n),
                       "%s %s: window against R1" % (name, kind))
        # a window two rows short on each side of what the output needs: the missing rows are special in the full map
        m2, _ = SV.case_map(O, kind, gin, gout, mode, seed=8, rows=(s_lo, s_lo + 1, s_hi - 2, s_hi - 1))
        short = m2[:, s_lo + 2:s_hi - 2]
        win = O.reproject(wi, si, short, wo, so, src_row0=s_lo + 2, src_nrows=s_hi - s_lo - 4, dst_row0=lo, dst_nrows=n)
        zeroed = m2.copy()
        zeroed[:, :s_lo + 2] = 0.0
        zeroed[:, s_hi - 2:] = 0.0
        SV.assert_same(win, O.reproject(wi, si, zeroed, wo, so)[:, lo:lo + n], "%s %s: rows outside the window read as 0.0" % (name, kind))
        SV.assert_same(win, SV.r1_reproject(O, wi, si, short, wo, so, src_row0=s_lo + 2, dst_row0=lo, dst_nrows=n),
                       "%s %s: short window against R1" % (name, kind))


@pytest.mark.parametrize("kind", SV.KINDS)
def test_sample_matches_written_definition(pj, O, kind):
    cases = SV.car_cases(pj)
    rng = np.random.default_rng(11)
    for name, mode in (("identity", "placed"), ("half_pixel_shift", "sprinkled"), ("sub_box_onto_full_sky", "placed")):
        (si, wi) = cases[name][0]
        for f32 in (False, True):
            m, mask = SV.special_map(kind, si, nc=2, seed=3, f32=f32, mode=mode)
            sky = SV.sky_points(rng, si, wi, mask)
            if f32:
                got = O.sample_bilinear_f32(wi, (si[0], si[1], 2), m, sky)
                exp = SV.to_f32(SV.r1_sample(O, wi, si, m.astype(np.float64), sky))
            else:
                got = O.sample_bilinear(wi, (si[0], si[1], 2), m, sky)
                exp = SV.r1_sample(O, wi, si, m, sky)
            SV.assert_same(got, exp, "sample %s %s f32=%s" % (name, kind, f32))
        # a row window: cells that straddle its edges, and an empty one
        m, mask = SV.special_map(kind, si, nc=1, seed=4, mode=mode, rows=(100, 149))
        sky = SV.sky_points(rng, si, wi, mask)
        for r0, nr in ((100, 50), (si[1] - 1, 1), (40, 0)):
            got = O.sample_bilinear(wi, (si[0], si[1], 1), m[:, r0:r0 + nr], sky, src_row0=r0, src_nrows=nr)
            SV.assert_same(got, SV.r1_sample(O, wi, si, m[:, r0:r0 + nr], sky, src_row0=r0), "sample window %s %s %s" % (name, kind, (r0, nr)))


def _generic_r1(O, win, proj_in, shape_in, src, wout, proj_out, shape_out):
    """pxl_reproject_generic_bilinear_f64_cpu restated: coordinates from the oracle's evaluators (pinned elsewhere), the gather
    from R1, a point behind the source's tangent plane reads as 0 (NaN only when its coordinates are not finite).  The
    visibility cosine uses math.sin / math.cos (the C library the oracle calls)."""
    nxo, nyo = shape_out
    jj, ii = np.meshgrid(np.arange(1, nyo + 1, dtype=float), np.arange(1, nxo + 1, dtype=float), indexing="ij")
    ip, jp = ii.ravel(), jj.ravel()
    if proj_out == 1:
        ra, dec = O.pix2sky_tan(wout, ip, jp)
    else:
        u = wout.unit
        ra = wout.crval[0] * u + (ip - wout.crpix[0]) * (wout.cdelt[0] * u)
        dec = wout.crval[1] * u + (jp - wout.crpix[1]) * (wout.cdelt[1] * u)
    visible = np.ones(len(ra), bool)
    if proj_in == 1:
        x, y = O.sky2pix_tan(win, ra, dec)
        a0, d0 = win.crval[0] * (math.pi / 180), win.crval[1] * (math.pi / 180)
        visible = np.array([(math.sin(d0) * math.sin(d) + math.cos(d) * math.cos(a - a0) * math.cos(d0)) > 0.0 for a, d in zip(ra, dec)])
        periodic = False
    else:
        x, y = O.sky2pix_soa(win, shape_in, ra, dec, safe=True, form=O.FORM_DIV)
        periodic = O.is_periodic(win, shape_in[0])
    v = SV.r1_bilerp(src, shape_in, x, y, periodic)
    v = np.where((~visible & np.isfinite(x) & np.isfinite(y))[None], 0.0, v)      # not visible: 0 whatever the map holds there
    return v.reshape(src.shape[0], nyo, nxo), visible.reshape(nyo, nxo)


@pytest.mark.parametrize("kind", SV.KINDS)
def test_reproject_generic_matches_written_definition(pj, O, kind):
    for name, (gin, pin, gout, pout) in SV.generic_cases(pj).items():
        (si, wi), (so, wo) = gin, gout
        for mode in ("placed", "sprinkled"):
            m, mask = SV.special_map(kind, si, nc=1, seed=5, mode=mode)
            got = O.reproject_generic(wi, pin, si, m, wo, pout, so)
            exp, visible = _generic_r1(O, wi, pin, si, m, wo, pout, so)
            SV.assert_same(got, exp, "generic %s %s %s" % (name, kind, mode))
            if pin == 1:
                assert (~visible).any() and visible.any()
                assert not got[0][~visible & ~np.isnan(got[0])].any()


# ---- the tests of the device file must not pass vacuously: conditions on its maps, from the oracle alone ----------------------
@pytest.mark.parametrize("kind", SV.NONFINITE)
def test_sprinkled_maps_reach_enough_outputs(pj, O, kind):
    """Every sprinkled case: the oracle's output has at least 5 % non-finite and at least 50 % finite elements."""
    for name, (gin, gout, mode) in SV.car_cases(pj).items():
        if mode != "sprinkled":
            continue
        (si, wi), (so, wo) = gin, gout
        for f32 in (False, True):
            m, mask = SV.case_map(O, kind, gin, gout, mode, seed=SV.case_seed(name), f32=f32)
            out = O.reproject_f32(wi, si, m, wo, so) if f32 else O.reproject(wi, si, m, wo, so)
            inside = np.ones(out.shape, bool)
            if name == "wide_box_to_fullsky":              # the box covers part of the sky: count inside its footprint
                inside = O.reproject(wi, si, np.ones(m.shape), wo, so) > 0
            bad = ~np.isfinite(out[inside])
            assert bad.mean() >= 0.05, (name, kind, f32, bad.mean())
            assert (~bad).mean() >= 0.5, (name, kind, f32, bad.mean())


@pytest.mark.parametrize("kind", SV.KINDS)
def test_placed_maps_have_zero_weight_special_taps(pj, O, kind):
    """Every placed case: some output pixel reads a special in-map tap with a weight of exactly zero (from the oracle's tables);
    for the non-finite kinds the oracle's output is NaN there."""
    for name, (gin, gout, mode) in SV.car_cases(pj).items():
        if mode != "placed":
            continue
        (si, wi), (so, wo) = gin, gout
        m, mask = SV.case_map(O, kind, gin, gout, mode, seed=SV.case_seed(name))
        xs, ys = O.reproject_tables(wi, si, wo, so)
        assert SV.zero_weight_special_taps(xs, ys, mask, O.is_periodic(wi, si[0])) > 0, (name, kind)
        if kind in SV.NONFINITE:
            out = O.reproject(wi, si, m, wo, so)
            assert np.isnan(out).any() and np.isfinite(out).mean() >= 0.5, (name, kind)


def test_same_reports_what_differs():
    a = np.array([1.0, -0.0, np.nan, np.inf, 5e-324])
    assert SV.same(a, a.copy())[0]
    assert SV.same(a, np.array([1.0, -0.0, -np.nan, np.inf, 5e-324]))[0]          # the sign of a NaN is not compared
    ok, msg = SV.same(a, np.array([1.0, 0.0, np.nan, np.inf, 5e-324]))
    assert not ok and "-0.0" in msg and "0x8000000000000000" in msg
    assert not SV.same(a, np.array([1.0, -0.0, np.nan, np.inf, 0.0]))[0]
    assert not SV.same(a, np.array([1.0, -0.0, 2.0, np.inf, 5e-324]))[0]
    f = a.astype(np.float32)
    assert SV.same(f, f.copy())[0] and not SV.same(f, -f)[0] and not SV.same(f, a)[0]
