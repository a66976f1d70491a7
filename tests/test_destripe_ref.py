"""tests/destripe_ref.py, the yardstick of the destriper, held to the dense matrices of its definition, and the
parts of the feature that need no device: the argument refusals of the two C entries and the public surface.  CPU only.

The refusal calls pass HOST buffers to the raw library: they are made only where pxl_device_count() is 0, so that a wrongly
accepted call can never launch (tests/test_abi_point_args.py's rule)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import destripe_ref as DR
import pointing_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PXL_EINVAL, PXL_EHIP = -22, -5


@pytest.fixture(scope="module")
def case(pj, O):
    """The end-to-end scan expanded with the numpy pointing yardstick: (scan, dense, tod with offsets)."""
    scan = DR.Scan(pj)
    qb, qd = scan.quaternions(pj, O)
    e = pointing_ref.expand(qb.numpy(), qd.numpy())
    sky, resp = np.stack([e["ra"], e["dec"]], axis=1), np.stack([e["q"], e["u"]], axis=1)
    return scan, scan.dense(O, sky, resp), scan.tod(O, sky, resp), sky, resp


def test_every_pixel_of_the_case_is_solved(case):
    """At rcond_min = 1e-3 no pixel of the end-to-end case is left out, so no test of it can pass by cutting pixels."""
    scan, dense, _tod, _sky, _resp = case
    print("min rcond %.3g, samples cut %d of %d" % (dense.rcond.min(), (~dense.live).sum(), dense.live.size))
    assert dense.solved.all() and 0 < (~dense.live).sum() < dense.live.size // 10
    assert dense.rcond.min() >= scan.RCOND_MIN


def test_the_operator_is_the_dense_one_and_symmetric(case):
    """bin -> block solve -> project, column by column, is F^T W Z F built from dense P, F and W; the matrix is symmetric,
    positive semi-definite, and its null space is the one constant offset.  Tolerance: both sides are Float64 sums of a few
    hundred terms of size |A|max, and the dense side goes through a pseudo-inverse of blocks with condition up to 1 / rcond_min:
    1e-10 |A|max leaves three orders over 600 x 2^-53 x 1e3."""
    _scan, dense, _tod, _sky, _resp = case
    _P, _F, _W, _Z, A = dense.matrices()
    n = A.shape[0]
    cols = np.stack([dense.apply(np.eye(n)[i]) for i in range(n)], axis=1)
    scale = np.abs(A).max()
    print("|apply - dense| max %.3g, asymmetry %.3g, of |A| max %.3g" % (np.abs(cols - A).max(), np.abs(cols - cols.T).max(), scale))
    assert np.abs(cols - A).max() <= 1e-10 * scale
    assert np.abs(cols - cols.T).max() <= 1e-10 * scale
    ev = np.linalg.eigvalsh((A + A.T) / 2)
    print("eigenvalues: %.3g, %.3g ... %.3g" % (ev[0], ev[1], ev[-1]))
    assert abs(ev[0]) <= 1e-10 * ev[-1] and ev[1] > 1e-6 * ev[-1]
    assert np.abs(A @ np.ones(n)).max() <= 1e-10 * scale


def test_it_recovers_the_sky_and_the_offsets(pj, case):
    """Noiseless samples of a random sky plus offsets of rms 5: the destriped map is the sky (I up to its mean) and the baselines
    are the offsets up to one constant, to 1e-5 -- tol = 1e-8 on the preconditioned residual times the offsets' norm
    (5 x sqrt(68)) times the operator's condition (a few tens) is 2e-5 at worst; the binned map of the same data is off by order 1."""
    scan, dense, tod, _sky, _resp = case
    m, a, info = dense.destripe(pj, tod, scan.TOL, scan.MAXITER)
    err = DR.map_error(m, scan.m0, dense.solved)
    da = (a - a.mean()) - (scan.a0 - scan.a0.mean())
    binned = DR.map_error(dense.solve_map(d=tod.reshape(-1)), scan.m0, dense.solved)
    print("iterations %d, map error %.3g, baseline error %.3g, binned map error %.3g" % (info["iterations"], err, np.abs(da).max(), binned))
    assert info["converged"] and not info["breakdown"]
    assert err <= 1e-5 and np.abs(da).max() <= 1e-5
    assert binned > 1000 * err
    # no offsets: the right-hand side is rounding alone.  CG solves for that rounding, whose component along the null vector (the
    # constant offset) is not small against the rest of it, so the baselines come back as ONE constant -- pure gauge, it moves
    # only the mean of I.  Apart from it they and the map are held to the bound of the case with offsets, which carries more
    m1, a1, _info = dense.destripe(pj, scan.tod(case[1].O, case[3], case[4], offsets=False), scan.TOL, scan.MAXITER)
    print("no offsets: baselines mean %.3g, spread %.3g" % (a1.mean(), np.abs(a1 - a1.mean()).max()))
    assert np.abs(a1 - a1.mean()).max() <= 1e-5 and DR.map_error(m1, scan.m0, dense.solved) <= 1e-5
    # a right-hand side that is exactly zero: pcg's rz0 == 0, zero baselines and the binned map (zeros here)
    m2, a2, info2 = dense.destripe(pj, np.zeros_like(tod), scan.TOL, scan.MAXITER)
    assert info2["iterations"] == 0 and info2["converged"] and not a2.any() and not m2.any()


def test_cut_samples_and_segment_sums(O, pj):
    """The yardstick's own rules on a handful of samples: the three forms of the sample value, a cut by position, by the map's
    edge and by the mask, a NaN d at a cut sample, and the baseline of each sample across a chunk that starts inside a baseline."""
    shape, wcs = pj.geometry([[6 * math.pi / 180, -6 * math.pi / 180], [-3 * math.pi / 180, 3 * math.pi / 180]], 0.5 * math.pi / 180)
    nx, ny = shape
    pix = np.array([[1.0, 1.0], [2.0, 1.0], [3.0, 2.0], [-5.0, 1.0], [4.0, 2.0], [5.0, 3.0], [6.0, 3.0], [7.0, 3.0]])
    sky = O.pix2sky(wcs, pix, O.WRAP_NONE)
    sky[4] = [np.nan, 0.0]
    mask = np.ones((ny, nx))
    mask[2, 5] = 0.0                                                         # pixel (6, 3): sample 6
    resp = np.tile([0.5, -0.25], (8, 1))
    w = np.arange(1.0, 9.0)
    d = np.arange(10.0, 18.0)
    d[[3, 4, 6]] = np.nan                                                    # every cut sample carries a NaN
    a = np.array([100.0, 200.0, 300.0, 400.0])                               # 2 detectors x 2 baselines of 5 samples
    args = (O, wcs, shape, sky, resp, w, 2, 3, 5, 2)                         # chunk: times 3..6 of each detector
    ch = DR.Chunk(O, wcs, shape, sky, w, 2, 3, 5, 2, d=d, a=a, mask=mask)
    assert list(ch.live) == [True, True, True, False, False, True, False, True]
    assert list(ch.b) == [0, 0, 1, 1, 2, 2, 3, 3]
    ref, n, S, touched = DR.project(*args, d=d, a=a, mask=mask)
    assert list(ref) == [1 * (10 - 100) + 2 * (11 - 100), 3 * (12 - 200), 6 * (15 - 300), 8 * (17 - 400)] and list(n) == [2, 1, 1, 1]
    ref, n, S, touched = DR.project(*args, a=a, mask=mask)
    assert list(ref) == [300.0, 600.0, 1800.0, 3200.0]
    rhs, k, _S = DR.bin(*args, d=d, mask=mask)
    assert np.isfinite(rhs).all() and k[0].sum() == 5 and rhs[0, 0, 0] == 10.0 and rhs[1, 0, 1] == 0.5 * 22.0 and rhs[2, 2, 6] == -0.25 * 8 * 17


# ---- the C entries' refusals --------------------------------------------------------------------------------------------------------

NX, NY, ND, NCHUNK, T0, BLEN, NBASE = 16, 9, 2, 4, 3, 5, 2


@pytest.fixture(scope="module")
def lib(pj):
    lib = pj.load_library()
    if lib.pxl_device_count() > 0:
        pytest.skip("a GPU is visible: these calls pass host pointers and may only run where no launch can succeed")
    return lib


class _Args:
    """A valid call of either entry on host buffers, every buffer a slot of one 64-byte aligned arena."""
    SLOTS = ("rhs3", "out", "map3", "mask", "sky", "resp", "w", "d", "a")

    def __init__(self):
        self.arena = np.zeros((len(self.SLOTS) + 1) * 1024)
        base = (self.arena.ctypes.data + 63) & ~63
        self.v = {s: base + i * 8192 for i, s in enumerate(self.SLOTS)}
        self.v.update(wcs="good", shape=[NX, NY, 3], n_det=ND, n_chunk=NCHUNK, t0=T0, baseline_len=BLEN, n_base=NBASE)

    def call(self, pj, lib, entry):
        from pixell_jl_amd._lib import CarWCSStruct
        v = self.v
        wcs = None
        if v["wcs"] is not None:
            wcs = CarWCSStruct()
            wcs.cdelt[0], wcs.cdelt[1], wcs.crpix[0], wcs.crpix[1] = -22.5, 22.5, 8.5, 5.0
            wcs.crval[0], wcs.crval[1], wcs.unit = 11.25, 0.0, math.pi / 180
        head = [None if wcs is None else C.byref(wcs), None if v["shape"] is None else (C.c_int64 * 3)(*v["shape"])]
        layout = [v[k] for k in ("n_det", "n_chunk", "t0", "baseline_len", "n_base")]
        tail = [v[k] for k in ("sky", "resp", "w", "d", "a")]
        if entry == "bin":
            rc = lib.pxl_baseline_bin_car_pol_nearest_f64(*head, v["rhs3"], v["mask"], *layout, *tail, None)
        else:
            rc = lib.pxl_baseline_project_car_pol_nearest_f64(*head, v["map3"], v["mask"], *layout, *tail, v["out"], None)
        return rc, pj._lib.last_error() if rc else ""


def _mutated(**changes):
    a = _Args()
    for k, val in changes.items():
        a.v[k] = a.v[val[1:]] if isinstance(val, str) and val.startswith("@") else val
    return a


REFUSALS = [
    ("both_null", dict(d=None, a=None), "d and a"),
    ("n_det_negative", dict(n_det=-1), "n_det"),
    ("n_chunk_negative", dict(n_chunk=-1), "n_chunk"),
    ("t0_negative", dict(t0=-1), "t0"),
    ("n_base_negative", dict(n_base=-1), "n_base"),
    ("baseline_len_zero", dict(baseline_len=0), "baseline_len"),
    ("baseline_len_negative", dict(baseline_len=-5), "baseline_len"),
    ("chunk_past_n_base", dict(n_base=1), "n_base"),
    ("t0_overflows", dict(t0=2 ** 63 - 2), "t0 + n_chunk"),
    ("n_overflows", dict(n_det=2 ** 40, n_chunk=2 ** 40, baseline_len=2 ** 41), "n_det * n_chunk"),
    ("bytes_overflow", dict(n_det=2 ** 30, n_chunk=2 ** 30, baseline_len=2 ** 31), "n_det * n_chunk"),
    ("n_base_overflows", dict(n_det=2 ** 31, n_chunk=1, n_base=2 ** 40), "n_det * n_base"),
    ("wcs_null", dict(wcs=None), "WCS"),
    ("shape_null", dict(shape=None), "shape"),
    ("nx_zero", dict(shape=[0, NY, 3]), "positive"),
    ("four_components", dict(shape=[NX, NY, 4]), "3 components"),
    ("sky_null", dict(sky=None), "null"),
    ("resp_null", dict(resp=None), "response"),
    ("w_null", dict(w=None), "null"),
]
BIN_ONLY = [
    ("rhs3_null", dict(rhs3=None), "null"),
    ("rhs3_on_sky", dict(rhs3="@sky"), "overlaps"),
    ("rhs3_on_resp", dict(rhs3="@resp"), "overlaps"),
    ("rhs3_on_w", dict(rhs3="@w"), "overlaps"),
    ("rhs3_on_d", dict(rhs3="@d"), "overlaps"),
    ("rhs3_on_a", dict(rhs3="@a"), "overlaps a"),
    ("rhs3_on_mask", dict(rhs3="@mask"), "overlaps mask"),
]
PROJECT_ONLY = [("out_null", dict(out=None), "null")] + [("out_on_" + k, dict(out="@" + k), "out overlaps")
                                                         for k in ("sky", "resp", "w", "d", "a", "map3", "mask")]


@pytest.mark.parametrize("entry", ["bin", "project"])
def test_the_entries_refuse_with_a_text_that_names_the_argument(pj, lib, entry):
    table = REFUSALS + (BIN_ONLY if entry == "bin" else PROJECT_ONLY)
    wrong = {}
    for name, changes, word in table:
        rc, text = _mutated(**changes).call(pj, lib, entry)
        if rc != PXL_EINVAL or word not in text or not text.startswith("baseline_" + entry):
            wrong[name] = (rc, text)
    assert not wrong, wrong
    a = _mutated(sky=_Args().v["sky"])
    a.v["sky"] += 8
    rc, text = a.call(pj, lib, entry)
    assert rc == PXL_EINVAL and "16-byte aligned" in text


@pytest.mark.parametrize("entry", ["bin", "project"])
def test_valid_and_empty_calls(pj, lib, entry):
    """A call that passes every check reaches its kernel (PXL_EHIP: there is no device); every allowed null is accepted; a call
    with no samples returns 0 before that."""
    for changes in (dict(), dict(mask=None), dict(d=None), dict(a=None), dict(map3=None), dict(t0=0, n_chunk=BLEN * NBASE)):
        rc, text = _mutated(**changes).call(pj, lib, entry)
        assert rc == PXL_EHIP and text.startswith("launch of k_baseline_" + entry), (changes, rc, text)
    for changes in (dict(n_det=0), dict(n_chunk=0), dict(n_chunk=0, n_base=0, t0=10 ** 6)):
        assert _mutated(**changes).call(pj, lib, entry) == (0, ""), changes


# ---- the surface ----------------------------------------------------------------------------------------------------------------------

def test_the_new_names_are_exported_and_bound(pj):
    for name in ("baseline_bin_pol_nearest", "baseline_project_pol_nearest", "destripe_map_pol_nearest_tod"):
        assert callable(getattr(pj, name))
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pixell_hip.h").read(), flags=re.S)
    julia = open(ROOT + "/julia/PixellHIP.jl").read()
    for name in ("pxl_baseline_bin_car_pol_nearest_f64", "pxl_baseline_project_car_pol_nearest_f64"):
        assert name in header and name in pj._lib.SIGNATURES and ":" + name in julia
    assert len(pj._lib.SIGNATURES["pxl_baseline_bin_car_pol_nearest_f64"][1]) == 15
    assert len(pj._lib.SIGNATURES["pxl_baseline_project_car_pol_nearest_f64"][1]) == 16
    for fn in ("baseline_bin!", "baseline_project!"):
        assert "function " + fn in julia and re.search(r"^export .*\b%s" % re.escape(fn), julia, flags=re.M)
