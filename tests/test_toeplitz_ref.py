"""tests/toeplitz_ref.py, the yardstick of the banded-Toeplitz noise weight, held to its dense matrix, and the parts
of the feature that need no device: the kernel builder and the reason for its taper, the refusals of the C entry and of the Python
wrappers, the public surface, and the ML map of the shared case (tests/ml_map_case.py) in its dense numpy form.  CPU only.

The refusal calls pass HOST buffers to the raw library: they are made only where pxl_device_count() is 0, so that a wrongly
accepted call can never launch (tests/test_abi_point_args.py's rule)."""
import functools
import os
import re

import numpy as np
import pytest
from host_arena import lib, mutated

import ml_map_case as MC
import toeplitz_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PXL_EINVAL, PXL_EHIP = -22, -5
EPS = 2.0 ** -52


# ---- the yardstick against the dense matrix ----------------------------------------------------------------------------------------

def _tiny(lam, seed):
    """One detector, 90 samples, three segments with gaps around them, 10 % cuts, a NaN under one of them."""
    rng = np.random.default_rng(seed)
    nt, seg = 90, [4, 30, 31, 70, 70, 84]
    x = rng.normal(size=(1, nt))
    w = (rng.uniform(0, 1, (1, nt)) >= 0.1).astype(np.float64)
    w[0, 40], x[0, 40] = 0.0, np.nan
    kern = rng.normal(size=(1, lam + 1)) / (1.0 + np.arange(lam + 1))
    return x, w, kern, seg


@pytest.mark.parametrize("lam", [0, 1, 3, 17, 64])
def test_the_float64_form_is_the_dense_matrix_product(lam):
    """Both forms of apply() against G T G x formed densely in long double, per sample within (lambda + 3) 2^-52 Sabs; the cut and
    the out-of-segment samples +0.0 by bits, the NaN under the cut nowhere."""
    x, w, kern, seg = _tiny(lam, 40 + lam)
    live = TR.live_mask(x.shape, seg, w)[0]
    A = TR.dense_gtg(kern[0], seg, live).astype(np.longdouble)
    want = A @ np.where(live, x[0], 0.0).astype(np.longdouble)
    bound = TR.bound(x, kern, seg, w)[0]
    for dtype in (np.float64, np.longdouble):
        got = TR.apply(x, kern, seg, w, dtype=dtype)[0]
        err = np.abs(got - want).astype(np.float64)
        print("lambda %d %s: worst error / bound %.3g" % (lam, dtype.__name__, (err[live] / bound[live]).max()))
        assert np.isfinite(np.asarray(got, dtype=np.float64)).all() and (err <= bound).all()
        off = np.asarray(got, dtype=np.float64)[~live]
        assert not off.any() and not np.signbit(off).any()


@pytest.mark.parametrize("lam", [1, 17, 64])
def test_gtg_is_symmetric(lam):
    """<u, G T G v> = <G T G u, v>: each side is within sum |u| bound(v) (or |v| bound(u)) of the exact form."""
    x, w, kern, seg = _tiny(lam, 50 + lam)
    rng = np.random.default_rng(lam)
    u, v = rng.normal(size=x.shape), rng.normal(size=x.shape)
    ld = lambda a: np.asarray(a, dtype=np.longdouble)
    lhs, rhs = (ld(u) * ld(TR.apply(v, kern, seg, w))).sum(), (ld(TR.apply(u, kern, seg, w)) * ld(v)).sum()
    tol = float((np.abs(u) * TR.bound(v, kern, seg, w)).sum() + (np.abs(v) * TR.bound(u, kern, seg, w)).sum())
    print("lambda %d: asymmetry %.3g, bound %.3g" % (lam, abs(float(lhs - rhs)), tol))
    assert abs(float(lhs - rhs)) <= tol


def test_lambda_zero_is_a_diagonal_weight_and_segments_do_not_couple():
    x, w, kern, seg = _tiny(0, 3)
    live = TR.live_mask(x.shape, seg, w)
    assert np.array_equal(TR.apply(x, kern, seg, w)[live], (kern[0, 0] * x)[live])
    # a change inside one segment leaves the others' bits, at a lambda longer than every segment
    x, w, kern, seg = _tiny(64, 4)
    x2 = x.copy()
    x2[0, 31:70] += 1.0
    a, b = TR.apply(x, kern, seg, w), TR.apply(x2, kern, seg, w)
    outside = np.ones(x.shape[1], dtype=bool)
    outside[31:70] = False
    assert np.array_equal(a[0, outside].view(np.int64), b[0, outside].view(np.int64)) and not np.array_equal(a[0, ~outside], b[0, ~outside])


# ---- the kernel builder -------------------------------------------------------------------------------------------------------------

TAPER_CASE = dict(n_fft=4096, fknee=0.1, alpha=3.0, lam=16)         # chosen so that the plain truncation is indefinite


def _smallest_eigenvalue(kern):
    return float(np.linalg.eigvalsh(TR.dense_gtg(kern, [0, 400], np.ones(400, dtype=bool)))[0])


def test_the_bartlett_kernel_is_positive_definite_and_the_plain_truncation_is_not(pj):
    c = TAPER_CASE
    psd = MC.psd(c["n_fft"], 1.0, c["fknee"], c["alpha"])
    tapered = pj.noise_kernel_from_psd(psd, c["lam"]).numpy()
    plain = np.fft.irfft(1.0 / psd, n=c["n_fft"])[:c["lam"] + 1]
    assert np.array_equal(tapered, plain * (1.0 - np.arange(c["lam"] + 1) / (c["lam"] + 1)))
    lo_t, lo_p = _smallest_eigenvalue(tapered), _smallest_eigenvalue(plain)
    print("smallest eigenvalue of a 400-sample block: tapered %.4g, truncated without a taper %.4g" % (lo_t, lo_p))
    assert lo_t > 0 and lo_p < 0
    # the map case's own kernel, and one row per detector
    assert _smallest_eigenvalue(pj.noise_kernel_from_psd(MC.psd(), MC.LAMBDA).numpy()) > 0
    two = pj.noise_kernel_from_psd(np.stack([psd, 2 * psd]), c["lam"], n_fft=c["n_fft"])
    assert tuple(two.shape) == (2, c["lam"] + 1) and np.array_equal(two[0].numpy(), tapered) and np.array_equal(two[1].numpy(), tapered / 2)
    # white noise: c_0 = 1 / sigma^2 and nothing else
    white = pj.noise_kernel_from_psd(np.full(33, 4.0), 5).numpy()
    assert white[0] == 0.25 and np.abs(white[1:]).max() <= 1e-17


def test_the_kernel_builder_refuses_a_bad_spectrum(pj):
    good = MC.psd(64)
    for bad in (0.0, -1.0, np.nan, np.inf):
        p = good.copy()
        p[5] = bad
        with pytest.raises(ValueError, match="finite and > 0"):
            pj.noise_kernel_from_psd(p, 4)
    with pytest.raises(ValueError, match="n_fft"):
        pj.noise_kernel_from_psd(good, 4, n_fft=100)
    for lam in (-1, 33, 5000):
        with pytest.raises(ValueError, match="lam must be"):
            pj.noise_kernel_from_psd(good, lam)
    with pytest.raises(ValueError, match="array of floats"):
        pj.noise_kernel_from_psd(np.ones((2, 3, 4)), 1)


# ---- the C entry's refusals -------------------------------------------------------------------------------------------------------

ND, NT, NSEG, LAM = 3, 40, 4, 5
SLOTS = ("seg_start", "x", "wlive", "out", "kern")              # kern last: at lambda = 4096 it runs past its slot, into nothing


def _entry(lib, v):
    return lib.pxl_tod_toeplitz_f64(v["n_det"], v["n_t"], v["n_seg"], v["seg_start"], v["lam"], v["kern"], v["x"], v["wlive"], v["out"], None)


_mutated = functools.partial(mutated, SLOTS, dict(n_det=ND, n_t=NT, n_seg=NSEG, lam=LAM), _entry)

REFUSALS = [
    ("lambda_negative", dict(lam=-1), "lambda"),
    ("lambda_4097", dict(lam=4097), "lambda"),
    ("n_det_negative", dict(n_det=-1), "n_det"),
    ("n_t_negative", dict(n_t=-1), "n_t"),
    ("n_seg_negative", dict(n_seg=-1), "n_seg"),
    ("n_overflows", dict(n_det=2 ** 40, n_t=2 ** 40), "n_det * n_t"),
    ("bytes_overflow", dict(n_det=2 ** 30, n_t=2 ** 30), "n_det * n_t"),
    ("kern_bytes_overflow", dict(n_det=2 ** 50, n_t=1, lam=4096), "n_det * (lambda + 1)"),
    ("seg_bytes_overflow", dict(n_seg=2 ** 62), "n_seg"),
    ("x_null", dict(x=None), "null x"),
    ("out_null", dict(out=None), "null out"),
    ("kern_null", dict(kern=None), "null kern"),
    ("seg_start_null", dict(seg_start=None), "null seg_start"),
    ("x_misaligned", dict(x="@x+4"), "8-byte aligned"),
    ("kern_misaligned", dict(kern="@kern+4"), "8-byte aligned"),
    ("wlive_misaligned", dict(wlive="@wlive+2"), "8-byte aligned"),
    ("out_is_x", dict(out="@x"), "out overlaps x"),
    ("out_shifted_on_x", dict(out="@x+8"), "out overlaps x"),
    ("out_ends_in_x", dict(out="@x+-952"), "out overlaps x"),
    ("out_on_kern", dict(out="@kern"), "out overlaps kern"),
    ("out_on_kern_end", dict(out="@kern+136"), "out overlaps kern"),
    ("out_on_wlive", dict(out="@wlive+64"), "out overlaps wlive"),
    ("out_on_seg_start", dict(out="@seg_start+32"), "out overlaps seg_start"),
    # 2^31 blocks: ranges of many GiB that must lie apart, so plain addresses far from each other (never dereferenced: refused, and no device)
    ("grid_too_large", dict(n_det=2 ** 31, n_t=1, x=1 << 40, out=1 << 41, kern=1 << 42, seg_start=1 << 43, wlive=None), "too many for one launch"),
]


def test_the_entry_refuses_with_a_text_that_names_the_argument(pj, lib):
    wrong = {}
    for name, changes, word in REFUSALS:
        rc, text = _mutated(**changes).call(pj, lib)
        if rc != PXL_EINVAL or word not in text or not text.startswith("tod_toeplitz"):
            wrong[name] = (rc, text)
    assert not wrong, wrong


def test_valid_and_empty_calls(pj, lib):
    """A call that passes every check reaches its kernel (PXL_EHIP: there is no device), at a lambda of every instantiation, with
    and without wlive and segments, and with out directly behind x; a call with no samples returns 0 before that, whatever else it
    holds."""
    valid = [dict(), dict(wlive=None), dict(n_seg=0), dict(out="@x+960"),
             dict(n_det=2 ** 31 - 1, n_t=1, x=1 << 40, out=1 << 41, kern=1 << 42, seg_start=1 << 43, wlive=None)]   # the largest grid
    for changes in valid + [dict(lam=v) for v in (0, 1, 128, 129, 1024, 1025, 4096)]:
        rc, text = _mutated(**changes).call(pj, lib)
        assert rc == PXL_EHIP and text.startswith("launch of k_toeplitz"), (changes, rc, text)
    for changes in (dict(n_det=0), dict(n_t=0), dict(n_det=0, x=None, out=None, kern=None, seg_start=None), dict(n_t=0, out="@x")):
        assert _mutated(**changes).call(pj, lib) == (0, ""), changes


# ---- the surface and the wrappers' host checks ----------------------------------------------------------------------------------------

def test_the_new_names_are_exported_and_bound(pj):
    import ctypes as C
    for name in ("toeplitz_tod", "noise_kernel_from_psd", "ml_map_pol_nearest_tod"):
        assert callable(getattr(pj, name))
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pixell_hip.h").read(), flags=re.S)
    julia = open(ROOT + "/julia/PixellHIP.jl").read()
    name = "pxl_tod_toeplitz_f64"
    assert name in header and name in pj._lib.SIGNATURES and ":" + name in julia
    args = pj._lib.SIGNATURES[name][1]
    assert len(args) == 10 and args[4] is C.c_int64 and args[3] is C.c_void_p
    assert "function toeplitz!" in julia and re.search(r"^export .*\btoeplitz!", julia, flags=re.M)
    assert '@testset "toeplitz!' in open(ROOT + "/julia/test_pixellhip.jl").read()
    import inspect
    assert list(inspect.signature(pj.toeplitz_tod).parameters) == ["tod", "kernel", "seg_start", "w", "out"]
    assert list(inspect.signature(pj.ml_map_pol_nearest_tod).parameters) == [
        "tod", "w", "q_bore", "q_det", "gamma", "shape", "wcs", "kernel", "seg_start", "rcond_min", "tol", "maxiter", "chunk_t"]


def test_the_wrapper_makes_its_host_checks_before_it_needs_a_device(pj):
    import torch
    tod = torch.zeros((2, 50), dtype=torch.float64)
    kern = torch.ones((5,), dtype=torch.float64)
    for bad, word in (([0, 30, 20, 50], "non-decreasing"), ([-1, 20, 50], r"inside \[0, T\]"), ([0, 20, 51], r"inside \[0, T\]"),
                      ([], "at least one"), ([0.5, 20], "integers"), (torch.tensor([0.0, 20.0]), "integer")):
        with pytest.raises(ValueError, match=word):
            pj.toeplitz_tod(tod, kern, bad)
    for bad in (torch.ones((3, 5), dtype=torch.float64), torch.ones((2, 5, 1), dtype=torch.float64), torch.ones((2, 0), dtype=torch.float64),
                torch.tensor(1.0, dtype=torch.float64), [1.0, 0.5]):
        with pytest.raises(ValueError, match="kernel is a"):
            pj.toeplitz_tod(tod, bad)
    with pytest.raises(ValueError, match="takes Float64 kernel"):
        pj.toeplitz_tod(tod, kern.to(torch.float32))
    with pytest.raises(ValueError, match="lambda must be 0 to 4096"):
        pj.toeplitz_tod(tod, torch.ones((4098,), dtype=torch.float64))
    with pytest.raises(ValueError, match="out may not be tod"):
        pj.toeplitz_tod(tod, kern, out=tod)
    with pytest.raises(ValueError, match=r"tod is a \(D, T\) tensor"):
        pj.toeplitz_tod(tod[0], kern)
    for seg in (None, [0, 25, 50]):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            pj.toeplitz_tod(tod, kern, seg)                                     # good host arguments: the next check is the device's


# ---- the ML map of the shared case, dense ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ml(pj, O):
    return MC.case(pj, O)


def test_ml_case_is_well_conditioned(ml):
    s = ml.system()
    print("solved %d of %d pixels, smallest rcond %.3g, cond(A) %.3g, cond(M^-1/2 A M^-1/2) %.3g" % (
        s.solved.sum(), s.solved.size, s.rcond.min(), s.cond, s.pcond))
    assert s.solved.all() and s.rcond.min() > 100 * MC.RCOND_MIN
    assert s.pcond < 20
    assert np.isnan(ml.tod()).sum() == (ml.w == 0).sum() > 0.05 * ml.w.size      # every cut sample is a NaN in the timestream


def test_ml_case_noiseless_recovers_the_sky(ml):
    s = ml.system()
    m = s.solve(ml.tod())
    err, bar = float(np.abs(m - ml.m0).max()), 100 * EPS * s.cond * float(np.abs(ml.m0).max())
    print("noiseless: worst error %.3g, bar %.3g" % (err, bar))
    assert err <= bar


def test_ml_case_beats_the_binned_map_under_one_over_f_noise(ml):
    """Five fixed seeds of P(f) = sigma^2 (1 + (f_knee / f)^2): the ML map's rms error is below the white-noise binned map's in
    every one (the ratios: DESIGN 4.21)."""
    s = ml.system()
    for seed in MC.SEEDS:
        d = ml.tod(seed)
        e_ml, e_bin = ml.rms(s.solve(d), s.solved), ml.rms(s.binned(d), s.solved)
        print("seed %d: rms error ML %.4f, binned %.4f, ratio %.3f" % (seed, e_ml, e_bin, e_ml / e_bin))
        assert e_ml < e_bin
