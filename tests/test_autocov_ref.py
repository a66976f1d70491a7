"""tests/autocov_ref.py, the yardstick of the gappy autocovariance, held to the literal definition, and the parts of
the feature that need no device: the spectrum builder pj.noise_psd_from_autocov and the reason for its default, the refusals of the
C entry and of the Python wrappers, and the public surface.  CPU only.

The refusal calls pass HOST buffers to the raw library: they are made only where pxl_device_count() is 0, so that a wrongly
accepted call can never launch (tests/test_abi_point_args.py's rule)."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch
from host_arena import lib, mutated

import autocov_ref as AR
import fit_ref
import toeplitz_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PXL_EINVAL, PXL_EHIP = -22, -5
EPS = 2.0 ** -52


# ---- the yardstick against the literal definition -----------------------------------------------------------------------------------

def _brute(x, lam, seg, w):
    """sums in long double and pairs by the double loop over (t, k) of the definition, one detector at a time."""
    nd, nt = x.shape
    spans = fit_ref.clamp(seg, nt)
    live = TR.live_mask(x.shape, seg, w)
    s = np.zeros((nd, lam + 1), dtype=np.longdouble)
    n = np.zeros((nd, lam + 1), dtype=np.int64)
    for det in range(nd):
        for lo, hi in spans:
            for t in range(lo, hi):
                for k in range(lam + 1):
                    if t + k < hi and live[det, t] and live[det, t + k]:
                        s[det, k] += np.longdouble(x[det, t]) * np.longdouble(x[det, t + k])
                        n[det, k] += 1
    return s, n


@pytest.mark.parametrize("seed", [0, 1])
def test_the_yardstick_is_the_double_loop_of_the_definition(seed):
    """T = 40, three segments with gaps around them and an empty one, 20 % cuts with NaN and Inf under them, every lambda from 0 to
    T: pairs equal, both forms of sums within bound of the long double loop; a lag with no pair is +0.0 and 0."""
    rng = np.random.default_rng(seed)
    nt, seg = 40, [2, 13, 13, 14, 37]
    x = rng.normal(size=(2, nt)) + 3.0
    w = (rng.uniform(0, 1, (2, nt)) >= 0.2).astype(np.float64)
    w[0, 5], w[1, 20], w[1, 21] = 0.0, -1.0, np.nan
    x[0, 5], x[1, 20], x[1, 21] = np.nan, np.inf, -np.inf
    worst = 0.0
    for lam in range(nt + 1):
        want, n = _brute(x, lam, seg, w)
        assert (AR.pairs(x.shape, lam, seg, w) == n).all()
        bound = AR.bound(x, lam, seg, w)
        for dtype in (np.float64, np.longdouble):
            got = AR.sums(x, lam, seg, w, dtype=dtype)
            err = np.abs(got - want).astype(np.float64)
            assert np.isfinite(np.asarray(got, dtype=np.float64)).all() and (err <= bound).all(), (lam, dtype)
            worst = max(worst, float((err[n > 0] / bound[n > 0]).max()))
            empty = np.asarray(got, dtype=np.float64)[n == 0]
            assert not empty.any() and not np.signbit(empty).any()
    assert (n[:, 24:] == 0).all() and (n[:, 0] > 0).all()          # the longest segment has 23 samples
    print("worst error / bound %.3g" % worst)


def test_the_plan_and_the_form_edges():
    """plan() restates the host's choice: LPG the power of two that holds ceil((lambda + 1) / 5) lanes, P W = the tile."""
    assert [AR.plan(lam) for lam in (0, 4, 5, 16, 64, 639, 640, 4096)] == [
        (1, 5, 256), (1, 5, 256), (2, 10, 128), (4, 20, 64), (16, 80, 16), (128, 640, 2), (256, 1280, 1), (256, 1280, 1)]
    for lam in range(0, AR.LAMBDA_MAX + 1):
        lpg, W, P = AR.plan(lam)
        assert P * W == AR.TILE and (lpg == 256 or W >= lam + 1) and (lpg == 1 or 5 * (lpg // 2) < lam + 1)
    forms = lambda lam: (AR.plan(lam)[0], -(-(lam + 1) // AR.plan(lam)[1]))
    edges = [lam for lam in range(1, AR.LAMBDA_MAX + 1) if forms(lam) != forms(lam - 1)]
    assert sorted(set(edges) | {e - 1 for e in edges}) == list(AR.FORM_EDGES)


# ---- the spectrum --------------------------------------------------------------------------------------------------------------------

def _cosine_sum(s, n, n_fft, normalise):
    """psd_m of noise_psd_from_autocov's docstring as the literal cosine sum, before any floor."""
    lam = s.shape[-1] - 1
    r = s / n[:, :1] if normalise == "biased" else np.where(n > 0, s / np.maximum(n, 1), 0.0)
    k = np.arange(lam + 1)
    tap = (1.0 - k / (lam + 1)) * r
    m = np.arange(n_fft // 2 + 1)
    return tap[:, :1] + 2.0 * (tap[:, 1:, None] * np.cos(2 * np.pi * m[None, None, :] * k[None, 1:, None] / n_fft)).sum(axis=1)


def test_biased_is_non_negative_for_any_cuts_and_pairs_is_not(pj):
    """Twenty random-walk timestreams (a steep red spectrum) in four scans of 150, lambda = 48: cuts of 10, 30 and 50 %, a whole scan
    cut in every fourth.  Before the floor the "biased" spectrum is >= -(lambda + 2) 2^-52 r_0 in every row; the "pairs" spectrum
    goes below that in at least one (it does in all twenty, down to -0.69 r_0).  The function's result is the cosine sum where
    nothing is floored."""
    lam, n_fft, nt, seg = 48, 128, 600, [0, 150, 300, 450, 600]
    violated = 0
    for seed in range(20):
        rng = np.random.default_rng(seed)
        x = np.cumsum(rng.normal(size=(2, nt)), axis=1)
        w = (rng.uniform(0, 1, (2, nt)) >= (0.1, 0.3, 0.5)[seed % 3]).astype(np.float64)
        if seed % 4 == 0:
            w[:, 150:300] = 0.0
        s, n = AR.sums(x, lam, seg, w), AR.pairs(x.shape, lam, seg, w)
        r0 = s[:, 0] / n[:, 0]
        raw = _cosine_sum(s, n, n_fft, "biased")
        assert (raw.min(axis=1) >= -(lam + 2) * EPS * r0).all(), seed
        psd, n_floored = pj.noise_psd_from_autocov(s, n, n_fft)
        assert psd.shape == (2, n_fft // 2 + 1) and np.isfinite(psd).all() and (psd > 0).all()
        keep = raw >= 1e-3 * np.median(raw, axis=1, keepdims=True)
        assert np.allclose(psd[keep], raw[keep], rtol=0, atol=1e-12 * r0.max()) and (n_floored == (~keep).sum(axis=1)).all()
        rawp = _cosine_sum(s, n, n_fft, "pairs")
        violated += bool((rawp.min(axis=1) < -(lam + 2) * EPS * r0).any())
        if (np.median(rawp, axis=1) > 0).all():
            psdp, nfp = pj.noise_psd_from_autocov(s, n, n_fft, normalise="pairs")
            assert (psdp > 0).all() and (nfp == (rawp < 1e-3 * np.median(rawp, axis=1, keepdims=True)).sum(axis=1)).all()
        else:                                                                   # more than half a row below zero: nothing to floor to
            with pytest.raises(ValueError, match="median is not positive"):
                pj.noise_psd_from_autocov(s, n, n_fft, normalise="pairs")
    print("'pairs' went negative in %d of 20" % violated)
    assert violated >= 1


def test_white_noise_gives_a_flat_spectrum_whose_mean_is_the_variance(pj):
    """2 10^5 samples of unit white noise in scans of 2000, one in ten cut, lambda = 16.  The mean of the spectrum over all n_fft
    frequencies is r_0 = sums_0 / pairs_0 (the inverse transform at lag 0) to rounding.  Flat: a Bartlett estimate has the
    relative variance (2/3) (lambda + 1) / N of its own level (N live samples), here a standard deviation of 0.79 %; every one of
    the 33 values within five of them."""
    rng = np.random.default_rng(5)
    nt, lam = 200000, 16
    x = rng.normal(size=(1, nt))
    w = (rng.uniform(0, 1, (1, nt)) >= 0.1).astype(np.float64)
    seg = list(range(0, nt + 1, 2000))
    s, n = AR.sums(x, lam, seg, w), AR.pairs(x.shape, lam, seg, w)
    psd, n_floored = pj.noise_psd_from_autocov(s[0], n[0])
    assert psd.shape == (33,) and n_floored == 0                           # n_fft = 64 >= 2 (lambda + 1) = 34; one row in, one row out
    r0 = s[0, 0] / n[0, 0]
    full = np.concatenate([psd, psd[-2:0:-1]])
    assert abs(full.mean() - r0) <= 64 * EPS * r0
    sd = np.sqrt(2.0 / 3.0 * (lam + 1) / n[0, 0])
    print("white: r_0 %.4f, worst |psd / r_0 - 1| = %.3g (sd %.3g)" % (r0, np.abs(psd / r0 - 1).max(), sd))
    assert np.abs(psd / r0 - 1).max() <= 5 * sd


def test_ar1_gives_the_analytic_spectrum_under_the_fejer_kernel(pj):
    """x_t = 0.9 x_(t-1) + e_t, 2 10^5 samples in one segment, no cuts, lambda = 64, n_fft = 256: the expectation is the analytic
    autocovariance r_k = 0.9^k / (1 - 0.81) under the Bartlett taper, that is the analytic spectrum convolved with the Fejer kernel.
    Measured with this seed: the worst relative deviation over the 129 frequencies is 0.052 (a Bartlett estimate's standard
    deviation is sqrt((2/3) 65 / 2 10^5) = 1.5 % of its level); asserted with a margin of 2 for the one fixed seed: 0.104."""
    rng = np.random.default_rng(8)
    nt, lam, n_fft, phi = 200000, 64, 256, 0.9
    e = rng.normal(size=nt)
    x = np.empty(nt)
    x[0] = e[0] / np.sqrt(1 - phi * phi)
    for t in range(1, nt):
        x[t] = phi * x[t - 1] + e[t]
    x = x[None, :]
    s, n = AR.sums(x, lam, [0, nt]), AR.pairs(x.shape, lam, [0, nt])
    psd, n_floored = pj.noise_psd_from_autocov(s, n, n_fft)
    true = (phi ** np.arange(lam + 1) / (1 - phi * phi))[None, :]
    want = _cosine_sum(true, np.ones((1, lam + 1), dtype=np.int64), n_fft, "biased")
    dev = float(np.abs(psd / want - 1).max())
    print("AR(1): worst relative deviation %.4f" % dev)
    assert n_floored[0] == 0 and dev <= 0.104


# ---- the C entry's refusals -------------------------------------------------------------------------------------------------------

ND, NT, NSEG, LAM = 3, 40, 4, 5
SLOTS = ("seg_start", "x", "wlive", "sums", "pairs")


def _entry(lib, v):
    return lib.pxl_tod_autocov_f64(v["n_det"], v["n_t"], v["n_seg"], v["seg_start"], v["lam"], v["x"], v["wlive"], v["sums"], v["pairs"], None)


_mutated = functools.partial(mutated, SLOTS, dict(n_det=ND, n_t=NT, n_seg=NSEG, lam=LAM), _entry)
_FAR = dict(x=1 << 40, sums=1 << 41, pairs=None, seg_start=1 << 43, wlive=None)     # never dereferenced: refused, or no device

REFUSALS = [
    ("lambda_negative", dict(lam=-1), "lambda"),
    ("lambda_4097", dict(lam=4097), "lambda"),
    ("n_det_negative", dict(n_det=-1), "n_det"),
    ("n_t_negative", dict(n_t=-1), "n_t"),
    ("n_seg_negative", dict(n_seg=-1), "n_seg"),
    ("n_overflows", dict(n_det=2 ** 40, n_t=2 ** 40), "n_det * n_t"),
    ("bytes_overflow", dict(n_det=2 ** 30, n_t=2 ** 30), "n_det * n_t"),
    ("sums_bytes_overflow", dict(n_det=2 ** 50, n_t=1, lam=4096), "n_det * (lambda + 1)"),
    ("seg_bytes_overflow", dict(n_seg=2 ** 62), "n_seg"),
    ("x_null", dict(x=None), "null x"),
    ("sums_null", dict(sums=None), "null sums"),
    ("seg_start_null", dict(seg_start=None), "null seg_start"),
    ("x_misaligned", dict(x="@x+4"), "8-byte aligned"),
    ("sums_misaligned", dict(sums="@sums+4"), "8-byte aligned"),
    ("pairs_misaligned", dict(pairs="@pairs+4"), "8-byte aligned"),
    ("wlive_misaligned", dict(wlive="@wlive+2"), "8-byte aligned"),
    ("sums_on_x", dict(sums="@x"), "sums overlaps x"),
    ("sums_ends_in_x", dict(sums="@x+-136"), "sums overlaps x"),
    ("sums_on_x_end", dict(sums="@x+952"), "sums overlaps x"),
    ("sums_on_wlive", dict(sums="@wlive+64"), "sums overlaps wlive"),
    ("sums_on_seg_start", dict(sums="@seg_start+32"), "sums overlaps seg_start"),
    ("pairs_on_x", dict(pairs="@x+8"), "pairs overlaps x"),
    ("pairs_on_wlive", dict(pairs="@wlive"), "pairs overlaps wlive"),
    ("pairs_on_seg_start", dict(pairs="@seg_start"), "pairs overlaps seg_start"),
    ("pairs_is_sums", dict(pairs="@sums"), "pairs overlaps sums"),
    ("pairs_on_sums_end", dict(pairs="@sums+136"), "pairs overlaps sums"),
    ("grid_too_large", dict(n_det=2 ** 31, n_t=1, **_FAR), "too many for one launch"),
]


def test_the_entry_refuses_with_a_text_that_names_the_argument(pj, lib):
    wrong = {}
    for name, changes, word in REFUSALS:
        rc, text = _mutated(**changes).call(pj, lib)
        if rc != PXL_EINVAL or word not in text or not text.startswith("tod_autocov"):
            wrong[name] = (rc, text)
    assert not wrong, wrong


def test_valid_and_empty_calls(pj, lib):
    """A call that passes every check reaches its kernel (PXL_EHIP: there is no device), at a lambda on both sides of every form,
    with and without wlive, pairs and segments, and with the outputs directly behind their neighbours.  No detectors: 0 and
    nothing else.  No samples but outputs: they are zeroed, so the call reaches the memset."""
    valid = [dict(), dict(wlive=None), dict(pairs=None), dict(n_seg=0), dict(sums="@x+960"), dict(pairs="@sums+144"),
             dict(n_det=2 ** 31 - 1, n_t=1, **_FAR)]                            # the largest grid
    big = dict(sums=1 << 41, pairs=1 << 42)                                    # rows of thousands of lags outgrow a slot
    for changes in valid + [dict(lam=v) for v in (0, 4, 5)] + [dict(lam=v, **big) for v in (639, 640, 1279, 1280, 4096)]:
        rc, text = _mutated(**changes).call(pj, lib)
        assert rc == PXL_EHIP and text.startswith("launch of k_autocov"), (changes, rc, text)
    for changes in (dict(n_det=0), dict(n_det=0, x=None, sums=None, pairs=None, seg_start=None), dict(n_det=0, n_t=0)):
        assert _mutated(**changes).call(pj, lib) == (0, ""), changes
    for changes in (dict(n_t=0), dict(n_t=0, x=None, seg_start=None, wlive=None, pairs=None)):
        rc, text = _mutated(**changes).call(pj, lib)
        assert rc == PXL_EHIP and text.startswith("hipMemsetAsync"), (changes, rc, text)
    rc, text = _mutated(n_t=0, pairs="@sums+8").call(pj, lib)                   # the outputs are still checked against each other
    assert rc == PXL_EINVAL and "pairs overlaps sums" in text


# ---- the surface and the wrappers' host checks ----------------------------------------------------------------------------------------

def test_the_new_names_are_exported_and_bound(pj):
    import ctypes as C
    for name in ("autocov_tod", "noise_psd_from_autocov", "noise_kernel_from_tod", "ml_map_pol_nearest_tod_auto"):
        assert callable(getattr(pj, name))
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pixell_hip.h").read(), flags=re.S)
    julia = open(ROOT + "/julia/PixellHIP.jl").read()
    name = "pxl_tod_autocov_f64"
    assert name in header and name in pj._lib.SIGNATURES and ":" + name in julia
    args = pj._lib.SIGNATURES[name][1]
    assert len(args) == 10 and args[4] is C.c_int64 and args[3] is C.c_void_p
    assert "function autocov!" in julia and re.search(r"^export .*\bautocov!", julia, flags=re.M)
    params = lambda f: list(inspect.signature(f).parameters)
    assert params(pj.autocov_tod) == ["tod", "lam", "seg_start", "w", "return_pairs"]
    assert params(pj.noise_psd_from_autocov) == ["sums", "pairs", "n_fft", "normalise", "floor"]
    assert params(pj.noise_kernel_from_tod) == ["tod", "lam", "seg_start", "w", "lam_est", "n_fft", "normalise", "floor"]
    assert params(pj.ml_map_pol_nearest_tod_auto) == [
        "tod", "w", "q_bore", "q_det", "gamma", "shape", "wcs", "lam", "seg_start", "lam_est", "n_fft", "n_pass", "normalise", "floor",
        "rcond_min", "tol", "maxiter", "chunk_t"]


def test_the_wrappers_make_their_host_checks_before_they_need_a_device(pj):
    tod = torch.zeros((2, 50), dtype=torch.float64)
    for bad, word in (([0, 30, 20, 50], "non-decreasing"), ([-1, 20, 50], r"inside \[0, T\]"), ([0, 20, 51], r"inside \[0, T\]"),
                      ([], "at least one"), ([0.5, 20], "integers"), (torch.tensor([0.0, 20.0]), "integer")):
        with pytest.raises(ValueError, match=word):
            pj.autocov_tod(tod, 4, bad)
    for bad in (-1, 4097, 1.5, True, None):
        with pytest.raises(ValueError, match="lam must be"):
            pj.autocov_tod(tod, bad)
        with pytest.raises(ValueError, match="lam must be"):
            pj.noise_kernel_from_tod(tod, bad)
        with pytest.raises(ValueError, match="lam must be"):
            pj.noise_kernel_from_tod(tod, 4, lam_est=bad if bad is not None else -2)
    with pytest.raises(ValueError, match=r"tod is a \(D, T\) tensor"):
        pj.autocov_tod(tod[0], 4)
    with pytest.raises(ValueError, match="takes Float64 tod"):
        pj.autocov_tod(tod.to(torch.float32), 4)
    for seg in (None, [0, 25, 50]):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            pj.autocov_tod(tod, 4, seg)                                         # good host arguments: the next check is the device's
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            pj.noise_kernel_from_tod(tod, 4, seg)


def test_the_spectrum_builder_refuses(pj):
    s, n = np.ones((2, 5)), np.full((2, 5), 7, dtype=np.int64)
    psd, nf = pj.noise_psd_from_autocov(torch.from_numpy(s), torch.from_numpy(n))
    assert psd.shape == (2, 9) and nf.shape == (2,)                             # n_fft = 16, the power of two >= 2 (lam + 1) = 10
    assert pj.noise_psd_from_autocov(s, n, n_fft=9)[0].shape == (2, 5)          # 2 lam + 1 holds the sequence
    for bad in (np.ones((2, 3, 4)), np.ones((2, 0)), np.ones((2, 5), dtype=np.int64)):
        with pytest.raises(ValueError, match="sums is a"):
            pj.noise_psd_from_autocov(bad, n)
    for bad in (n.astype(np.float64), n[:, :4], n[0]):
        with pytest.raises(ValueError, match="pairs is an array of integers"):
            pj.noise_psd_from_autocov(s, bad)
    for bad in (8, 2, 0, -16):
        with pytest.raises(ValueError, match="n_fft must exceed 2 lam"):
            pj.noise_psd_from_autocov(s, n, n_fft=bad)
    with pytest.raises(ValueError, match="normalise"):
        pj.noise_psd_from_autocov(s, n, normalise="unbiased")
    for bad in (0.0, 1.0, -1e-3, np.nan):
        with pytest.raises(ValueError, match="floor"):
            pj.noise_psd_from_autocov(s, n, floor=bad)
    n0 = n.copy()
    n0[1, 0] = 0
    with pytest.raises(ValueError, match="detector 1 has no live sample"):
        pj.noise_psd_from_autocov(s, n0)
    for bad in (np.nan, np.inf):
        s1 = s.copy()
        s1[1, 3] = bad
        with pytest.raises(ValueError, match="detector 1 has a non-finite sum"):
            pj.noise_psd_from_autocov(s1, n)
    n2 = n.copy()
    n2[0, 3] = 0                                                                # "pairs": a lag with no pair is +0.0, not a division by zero
    assert np.isfinite(pj.noise_psd_from_autocov(s, n2, normalise="pairs")[0]).all()


def test_the_map_maker_refuses_before_it_needs_a_device(pj):
    tod = torch.zeros((2, 50), dtype=torch.float64)
    args = (tod, torch.ones_like(tod), torch.zeros((50, 4), dtype=torch.float64), torch.zeros((2, 4), dtype=torch.float64), None, (8, 8), None)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="n_pass must be"):
            pj.ml_map_pol_nearest_tod_auto(*args, 4, n_pass=bad)
    for bad in (-1, 4097, 2.0):
        with pytest.raises(ValueError, match="lam must be"):
            pj.ml_map_pol_nearest_tod_auto(*args, bad)
        with pytest.raises(ValueError, match="lam must be"):
            pj.ml_map_pol_nearest_tod_auto(*args, 4, lam_est=bad)
    with pytest.raises(ValueError, match="normalise"):
        pj.ml_map_pol_nearest_tod_auto(*args, 4, normalise="none")
    for lam, lam_est, n_fft in ((4, 4, 8), (4, 16, 32), (16, 4, 16)):
        with pytest.raises(ValueError, match="n_fft must exceed"):
            pj.ml_map_pol_nearest_tod_auto(*args, lam, lam_est=lam_est, n_fft=n_fft)
