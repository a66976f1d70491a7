"""The distance-transform yardstick (tests/sdt_ref.py) against the reference's own testset, and the C entry's argument
checks, which run before any device work (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

import sdt_ref as R
from conftest import DEG


def _box(pj, ra1, ra2, dec1, dec2, res):
    return pj.geometry([[ra1 * DEG, ra2 * DEG], [dec1 * DEG, dec2 * DEG]], res * DEG)


def test_yardstick_passes_the_reference_metric_testset(pj):
    """test_distance_transform.jl:26-44: m[1,1] = 0 on the 0.5 degree box [20 -20; 0 10]; along the first row the distance is
    the RA offset, along the first column the DEC offset (Julia's scalar isapprox, rtol sqrt(eps))."""
    shape, wcs = _box(pj, 20, -20, 0, 10, 0.5)
    nx, ny = shape
    m = np.ones((ny, nx))
    m[0, 0] = 0.0
    dist = R.distance_transform(m, wcs)
    ra, dec = R.sky_angles(wcs, shape)
    rtol = np.sqrt(np.finfo(float).eps)
    for i in range(nx):
        a, b = ra[0] - ra[i], dist[0, i]
        assert abs(a - b) <= rtol * max(abs(a), abs(b)), i
    for j in range(ny):
        a, b = dec[j] - dec[0], dist[j, 0]
        assert abs(a - b) <= rtol * max(abs(a), abs(b)), j


def test_yardstick_sampled_form_equals_the_full_table(pj):
    """The sampled form with a DEC cap (the pruning the large-map tests use) gives the full table's values."""
    shape, wcs = pj.fullsky_geometry(4 * DEG)
    nx, ny = shape
    rng = np.random.default_rng(3)
    m = np.ones((ny, nx))
    m[rng.integers(0, ny, 12), rng.integers(0, nx, 12)] = 0.0
    full = R.distance_transform(m, wcs)
    jj, ii = np.divmod(rng.choice(nx * ny, 300, replace=False), nx)
    zj, zi = np.nonzero(m == 0)
    got = R.sampled(wcs, shape, ii, jj, zi, zj, cap=full[jj, ii])
    assert np.array_equal(got, full[jj, ii])


def test_bound_is_never_looser_than_the_ceiling():
    theta = np.concatenate([np.geomspace(1e-9, 3.1, 2000), [np.pi / 2, 3.14159]])
    b = R.bound(theta)
    assert (b <= 4e-15 / np.maximum(np.sin(theta), 1e-3) + 8 * np.spacing(theta)).all()
    assert (b > 0).all()


# ---- the masks of the device tests tell a right kernel from a subtly wrong one -----------------------------------------
# R.emulate is the device's method in numpy; each mutation is one line of it gone wrong.  The cases below are exactly the
# ones tests/test_gpu_distance_transform.py runs on the device (R.ALL_CASES), with the same brute-force reference.

_WRAPPING = ("cc4", "cc3", "fejer4", "gap4_dec_down")       # geometries where the way round the seam or gap can be shorter
CAUGHT_BY = {
    # a row with several zeros where the nearest lies round the seam or gap
    "no_wrap": tuple("dense/%s/staircase" % g for g in _WRAPPING) + tuple("dense/%s/half_plane" % g for g in _WRAPPING[:3])
    + ("far/antipodal_pair", "scan/z65535_65536", "scan/words_1024_up"),
    # a query between two zeros of one 64-column word, the left one nearer
    "own_word": R.WORD_EDGE_CASES + tuple("dense/%s/%s" % (g, k) for g in R.DENSE_GEOMETRIES
                                          for k in ("ellipse", "crossing_staircases"))
    + ("far/antipodal_pair", "scan/every_256"),
    # more than one row with a zero
    "sweep_inverted": R.DENSE_CASES + R.WORD_EDGE_CASES + ("far/antipodal_rows",),
    # a chain with a vertex to drop
    "no_pops": tuple("dense/%s/%s" % (g, k) for g in R.DENSE_GEOMETRIES for k in ("ellipse", "crossing_staircases"))
    + tuple("dense/%s/%s" % (g, k) for g in _WRAPPING for k in ("full_column", "staircase")) + ("far/antipodal_rows",),
}
# Cases no mutation of the emulation fails on.  They stay for paths only the device has: a single vertex of negative x
# (far/...), and the carries of the row scan's two trips, which the emulation replaces by a search
# (scan/z...: one zero on one side of a carry, so every word on the other side, and the row's first or last zero, needs it).
DEVICE_PATHS_ONLY = ("far/off_pole", "far/pole_row", "scan/z65535", "scan/z65536", "scan/z4479", "scan/z4480")


def test_every_case_is_caught_by_a_mutation_or_names_a_device_path():
    caught = set(c for cases in CAUGHT_BY.values() for c in cases)
    assert caught.isdisjoint(DEVICE_PATHS_ONLY)
    assert caught | set(DEVICE_PATHS_ONLY) == set(R.ALL_CASES)
    assert sorted(CAUGHT_BY) == sorted(R.MUTATIONS)


@pytest.mark.parametrize("name", R.ALL_CASES)
def test_emulation_is_within_the_bound(pj, name):
    """The method itself holds on every case: every pixel within the bound, zero pixels exactly +0.0."""
    m, shape, wcs, ref = R.case(pj, name)
    got = R.emulate(m, wcs)
    zero = m == 0
    assert np.array_equal(got[zero].view(np.int64), np.zeros(int(zero.sum()), np.int64))
    r = R.worst_ratio(got, ref)
    print("%s: emulation, worst error / bound = %.3g" % (name, r))
    assert r <= 1.0


@pytest.mark.parametrize("mutate,name", [(mu, c) for mu in R.MUTATIONS for c in CAUGHT_BY[mu]])
def test_mutation_exceeds_the_bound(pj, mutate, name):
    """Each mutation misses the bound on the cases named for it (by six orders of magnitude or more: a wrong zero, not a
    rounding)."""
    m, shape, wcs, ref = R.case(pj, name)
    with np.errstate(invalid="ignore"):
        got = R.emulate(m, wcs, mutate)
    got = np.where(np.isnan(got), np.inf, got)
    r = R.worst_ratio(got, ref)
    print("%s, %s: worst error / bound = %.3g" % (name, mutate, r))
    assert r > 1e6


def _c_entry(pj):
    lib = pj.load_library()
    return lib.pxl_distance_transform_car_f64


def _call(pj, wcs, shape, m_ptr, d_ptr):
    return _c_entry(pj)(C.byref(wcs.to_struct()) if wcs is not None else None, pj._lib.shape_arr(shape) if shape else None,
                        C.c_void_p(m_ptr), C.c_void_p(d_ptr), None)


def test_c_entry_rejects_bad_arguments_without_gpu(pj):
    """PXL_EINVAL with a message naming distance_transform, before any device work: invalid WCS, null pointers,
    non-positive shapes, overlapping buffers, a box running past a pole."""
    shape, wcs = _box(pj, 20, -20, -10, 10, 0.5)
    fake_m, fake_d = 1 << 20, 1 << 30                      # never dereferenced: every case fails its checks first
    cases = []
    cases.append(("invalid WCS", _c_entry(pj)(None, pj._lib.shape_arr(shape), C.c_void_p(fake_m), C.c_void_p(fake_d), None)))
    bad = pj.CarClenshawCurtis((0.0, 0.5), wcs.crpix, wcs.crval)
    cases.append(("zero cdelt", _call(pj, bad, shape, fake_m, fake_d)))
    cases.append(("null map", _call(pj, wcs, shape, 0, fake_d)))
    cases.append(("null output", _call(pj, wcs, shape, fake_m, 0)))
    cases.append(("null shape", _c_entry(pj)(C.byref(wcs.to_struct()), None, C.c_void_p(fake_m), C.c_void_p(fake_d), None)))
    cases.append(("empty shape", _call(pj, wcs, (0, shape[1]), fake_m, fake_d)))
    cases.append(("overlap", _call(pj, wcs, shape, fake_m, fake_m + 8)))
    polar_shape, polar = _box(pj, 20, -20, 80, 100, 0.5)     # rows above DEC = 90 degrees
    cases.append(("past a pole", _call(pj, polar, polar_shape, fake_m, fake_d)))
    for what, rc in cases:
        assert rc == -22, what
        msg = pj._lib.last_error()
        assert "distance_transform" in msg, (what, msg)
    assert "pole" in msg


@pytest.mark.parametrize("what", R.REFUSED)
def test_c_entry_refuses_geometry_without_gpu(pj, what):
    """The entry's four refusals of a geometry, each with its reason, before any device work."""
    shape, wcs, reason = R.refused_geometry(pj, what)
    assert _call(pj, wcs, shape, 1 << 20, 1 << 40) == -22
    msg = pj._lib.last_error()
    assert "distance_transform" in msg and reason in msg, msg


def test_julia_methods_are_one_per_concrete_sdt_type():
    """The reference defines distance_transform(::BruteForceSDT, ::Enmap), (::ApproxSeqSDT, ::Enmap) and
    (::ExactSeqSDT, ::Enmap) (transform_distance.jl:55, 193, 322).  A device method on ::AbstractSDT (or a Union of the
    three) would be ambiguous with each of them, so the binding defines one method per concrete type."""
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "julia", "PixellHIP.jl")).read()
    assert not re.search(r"distance_transform\(::(Pixell\.)?(AbstractSDT|Union)", text)
    loop = re.search(r"for DT in \(([^)]*)\)\s*\n\s*@eval Pixell\.distance_transform\(::Pixell\.\$DT, m::Enmap\{Float64,2,<:HIPArray,"
                     r"<:AbstractCARWCS\}\)", text)
    assert loop, "PixellHIP.jl lacks the per-type distance_transform methods"
    assert sorted(s.strip().lstrip(":") for s in loop.group(1).split(",")) == ["ApproxSeqSDT", "BruteForceSDT", "ExactSeqSDT"]
