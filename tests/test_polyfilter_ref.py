"""tests/polyfilter_ref.py, the yardstick of the per-scan polynomial filter, held to the properties of the
projection it defines, and the parts of the feature that need no device: the refusals of the C entry and of the Python wrapper,
the public surface, and the filter-and-bin case on the numpy composition.  CPU only.

The refusal calls pass HOST buffers to the raw library: they are made only where pxl_device_count() is 0, so that a wrongly
accepted call can never launch (tests/test_abi_point_args.py's rule)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
from host_arena import lib, mutated

import filter_bin_case as FB
import polyfilter_ref as PF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PXL_EINVAL, PXL_EHIP = -22, -5
EPS = 2.0 ** -52


def _weights(kind, shape, rng):
    return None if kind == "uniform" else rng.uniform(0.25, 4.0, shape)


# ---- the yardstick's own properties -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["uniform", "random"])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_it_annihilates_every_polynomial_up_to_the_order(kind, dtype):
    """d = a polynomial of degree <= order in the sample index: out is rounding in every segment, the one-sample segment (which
    is fitted with one coefficient) included, and the samples outside the segments are copied.  The bound: a pivot ratio r costs
    1 / r of the precision, and a fit is some tens of operations per coefficient: 100 eps / (the smallest accepted ratio) max|d|."""
    rng = np.random.default_rng(5)
    seg = [3, 20, 21, 60, 141, 150]
    nt = 160
    t = np.arange(nt, dtype=np.float64)
    for order in (0, 1, 3, 7):
        d = np.stack([sum(rng.normal() * (t / 40.0 - 1.5) ** p for p in range(order + 1)) for _ in range(2)])
        fit = PF.filter(d, seg, order, wfit=_weights(kind, d.shape, rng), dtype=dtype)
        full = [s for s, (lo, hi) in enumerate(PF.clamp_segments(seg, nt)) if hi - lo > order]
        assert (fit.n_used[:, full] == order + 1).all() and (fit.n_used[:, 1] == 1).all()
        rmin = float(np.nanmin(np.asarray(fit.ratios[:, full], dtype=np.float64)))
        out = np.asarray(fit.out, dtype=np.float64)
        resid = np.abs(out[:, seg[0]:seg[-1]]).max()
        print("order %d: smallest pivot ratio %.3g, residual %.3g of max|d| %.3g" % (order, rmin, resid, np.abs(d).max()))
        assert rmin > 1e-7 and resid <= 100 * EPS / rmin * np.abs(d).max()
        assert np.array_equal(out[:, :seg[0]], d[:, :seg[0]]) and np.array_equal(out[:, seg[-1]:], d[:, seg[-1]:])


@pytest.mark.parametrize("kind", ["uniform", "random"])
def test_it_is_idempotent(kind):
    """Z Z d = Z d: the second application changes a sample by rounding of the first's size."""
    rng = np.random.default_rng(6)
    seg = [0, 64, 65, 130, 400]
    d = rng.normal(size=(2, 400))
    w = _weights(kind, d.shape, rng)
    for order in (0, 2, 5):
        once = PF.filter(d, seg, order, wfit=w).out
        twice = PF.filter(once, seg, order, wfit=w)
        print("order %d: |ZZd - Zd| max %.3g, second coefficients max %.3g" % (order, np.abs(twice.out - once).max(), np.abs(twice.coeffs).max()))
        assert np.abs(twice.out - once).max() <= 1e4 * EPS * np.abs(d).max()
        assert np.abs(twice.coeffs).max() <= 1e4 * EPS * np.abs(d).max()


@pytest.mark.parametrize("kind", ["uniform", "random"])
def test_wz_is_symmetric_and_the_filter_is_the_dense_projector(kind):
    """One segment of 12 samples, order 3: the columns of the filter are Z = I - F (F^T W F)^-1 F^T W, and W Z is symmetric."""
    rng = np.random.default_rng(7)
    L, order = 12, 3
    w = np.ones(L) if kind == "uniform" else rng.uniform(0.25, 4.0, L)
    Z = np.stack([PF.filter(np.eye(L)[i][None], [0, L], order, wfit=w[None]).out[0] for i in range(L)], axis=1)
    dense = PF.projector(L, order, w)
    WZ = w[:, None] * Z
    print("|Z - dense| max %.3g, asymmetry of W Z %.3g" % (np.abs(Z - dense).max(), np.abs(WZ - WZ.T).max()))
    assert np.abs(Z - dense).max() <= 1e-12 and np.abs(WZ - WZ.T).max() <= 1e-12
    assert np.abs(Z @ Z - Z).max() <= 1e-12


def test_truncation_counts_the_live_samples():
    """A segment with n live samples and order >= n is fitted with exactly n coefficients, the rest +0.0, and its live samples come
    out as rounding; with no live sample it is copied, -0.0 and NaN included."""
    rng = np.random.default_rng(8)
    L = 40
    for order in (1, 3, 7):
        for n in range(0, order + 1):
            d = rng.normal(size=(1, L))
            d[0, 0], d[0, 1] = -0.0, np.nan
            w = np.zeros((1, L))
            live = 2 + rng.choice(L - 2, size=n, replace=False)
            w[0, live] = rng.uniform(0.5, 2.0, n)
            for dtype in (np.float64, np.longdouble):
                fit = PF.filter(d, [0, L], order, wfit=w, dtype=dtype)
                assert fit.n_used[0, 0] == n, (order, n, fit.ratios)
                assert not fit.coeffs[0, 0, n:].any() and not np.signbit(np.asarray(fit.coeffs[0, 0, n:], dtype=np.float64)).any()
                out = np.asarray(fit.out, dtype=np.float64)
                if n == 0:
                    assert np.array_equal(out.view(np.int64), d.view(np.int64))
                else:
                    # n coefficients interpolate n samples.  The residual there is the coefficients' error, and a solve loses
                    # 1 / (the smallest accepted ratio) of the precision of coefficients that, through irregular samples, are
                    # far larger than d: 100 eps sum|c| / min ratio
                    r = np.asarray(fit.ratios[0, 0], dtype=np.float64)
                    csum = float(np.abs(np.asarray(fit.coeffs[0, 0], dtype=np.float64)).sum())
                    assert np.isnan(out[0, 1]) and np.abs(out[0, live]).max() <= 100 * EPS / r[:n].min() * csum
                    assert r[:n].min() > 1e-10 and (n == order + 1 or not r[n] > 1e-10)


def test_the_group_rule_reaches_every_size():
    assert PF.group(1, 1, 0) == 1 and PF.group(5000, 1, 0) == 256 and PF.group(5000, 4, 7) == 256 and PF.group(5000, 5, 0) == 64
    assert sorted({PF.group(130, s, o) for s in range(1, 131) for o in range(8)}) == [1, 2, 4, 8, 16, 32, 64]


# ---- the C entry's refusals -------------------------------------------------------------------------------------------------------

ND, NT, NSEG, ORDER = 3, 40, 4, 2


SLOTS = ("seg_start", "d", "wfit", "out", "coeffs", "n_used")


def _entry(lib, v):
    return lib.pxl_tod_polyfilter_f64(v["n_det"], v["n_t"], v["n_seg"], v["seg_start"], v["order"], v["rcond_min"], v["d"], v["wfit"], v["out"],
                                      v["coeffs"], v["n_used"], None)


_mutated = functools.partial(mutated, SLOTS, dict(n_det=ND, n_t=NT, n_seg=NSEG, order=ORDER, rcond_min=1e-10), _entry)


REFUSALS = [
    ("order_negative", dict(order=-1), "order"),
    ("order_eight", dict(order=8), "order"),
    ("rcond_min_negative", dict(rcond_min=-1e-3), "rcond_min"),
    ("rcond_min_one", dict(rcond_min=1.0), "rcond_min"),
    ("rcond_min_nan", dict(rcond_min=float("nan")), "rcond_min"),
    ("n_det_negative", dict(n_det=-1), "n_det"),
    ("n_t_negative", dict(n_t=-1), "n_t"),
    ("n_seg_negative", dict(n_seg=-1), "n_seg"),
    ("n_overflows", dict(n_det=2 ** 40, n_t=2 ** 40), "n_det * n_t"),
    ("bytes_overflow", dict(n_det=2 ** 30, n_t=2 ** 30), "n_det * n_t"),
    ("segments_overflow", dict(n_det=2 ** 31, n_seg=2 ** 40), "n_det * n_seg"),
    ("coeff_bytes_overflow", dict(n_det=2 ** 29, n_seg=2 ** 29, order=7), "n_det * n_seg"),
    ("seg_bytes_overflow", dict(n_det=1, n_seg=2 ** 62), "n_det * n_seg"),
    ("d_null", dict(d=None), "null d"),
    ("out_null", dict(out=None), "null out"),
    ("seg_start_null", dict(seg_start=None), "null seg_start"),
    ("d_misaligned", dict(d="@d+4"), "8-byte aligned"),
    ("out_shifted_on_d", dict(out="@d+8"), "out overlaps d other than exactly"),
    ("out_on_wfit", dict(out="@wfit"), "out overlaps wfit"),
    ("out_on_seg_start", dict(out="@seg_start"), "out overlaps seg_start"),
    ("coeffs_on_d", dict(coeffs="@d"), "coeffs overlaps d"),
    ("coeffs_on_wfit", dict(coeffs="@wfit+64"), "coeffs overlaps wfit"),
    ("coeffs_on_seg_start", dict(coeffs="@seg_start"), "coeffs overlaps seg_start"),
    ("coeffs_on_out", dict(coeffs="@out"), "coeffs overlaps out"),
    ("n_used_on_d", dict(n_used="@d+16"), "n_used overlaps d"),
    ("n_used_on_wfit", dict(n_used="@wfit"), "n_used overlaps wfit"),
    ("n_used_on_seg_start", dict(n_used="@seg_start+8"), "n_used overlaps seg_start"),
    ("n_used_on_out", dict(n_used="@out"), "n_used overlaps out"),
    ("n_used_on_coeffs", dict(n_used="@coeffs+8"), "n_used overlaps coeffs"),
    ("coeffs_on_d_in_place", dict(out="@d", coeffs="@d"), "coeffs overlaps"),
]


def test_the_entry_refuses_with_a_text_that_names_the_argument(pj, lib):
    wrong = {}
    for name, changes, word in REFUSALS:
        rc, text = _mutated(**changes).call(pj, lib)
        if rc != PXL_EINVAL or word not in text or not text.startswith("tod_polyfilter"):
            wrong[name] = (rc, text)
    assert not wrong, wrong


def test_valid_and_empty_calls(pj, lib):
    """A call that passes every check reaches its kernel (PXL_EHIP: there is no device); every allowed null and the in-place form
    are accepted, at every order; a call with no samples returns 0 before that, whatever else it holds."""
    valid = [dict(), dict(wfit=None), dict(coeffs=None), dict(n_used=None), dict(out="@d"), dict(n_seg=0), dict(rcond_min=0.0)]
    for changes in valid + [dict(order=o) for o in range(8)]:
        rc, text = _mutated(**changes).call(pj, lib)
        assert rc == PXL_EHIP and text.startswith("launch of k_polyfilter"), (changes, rc, text)
    for changes in (dict(n_det=0), dict(n_t=0), dict(n_det=0, d=None, out=None, seg_start=None), dict(n_t=0, out="@wfit")):
        assert _mutated(**changes).call(pj, lib) == (0, ""), changes


# ---- the surface ------------------------------------------------------------------------------------------------------------------------

def test_the_new_names_are_exported_and_bound(pj):
    for name in ("polyfilter_tod", "filter_bin_map_pol_nearest_tod"):
        assert callable(getattr(pj, name))
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pixell_hip.h").read(), flags=re.S)
    julia = open(ROOT + "/julia/PixellHIP.jl").read()
    name = "pxl_tod_polyfilter_f64"
    assert name in header and name in pj._lib.SIGNATURES and ":" + name in julia
    assert len(pj._lib.SIGNATURES[name][1]) == 12
    assert pj._lib.SIGNATURES[name][1][4] is C.c_int and pj._lib.SIGNATURES[name][1][5] is C.c_double
    assert "function polyfilter!" in julia and re.search(r"^export .*\bpolyfilter!", julia, flags=re.M)
    assert '@testset "polyfilter!' in open(ROOT + "/julia/test_pixellhip.jl").read()


def test_the_wrapper_refuses_a_bad_seg_start_before_it_needs_a_device(pj):
    """The segment offsets are checked on the host, before the device checks: decreasing, below 0, past T, empty, not integers."""
    import torch
    tod = torch.zeros((2, 50), dtype=torch.float64)
    for bad, word in (([0, 30, 20, 50], "non-decreasing"), ([-1, 20, 50], r"inside \[0, T\]"), ([0, 20, 51], r"inside \[0, T\]"),
                      (torch.tensor([10, 5]), "non-decreasing"), ([], "at least one"), ([0.5, 20], "integers"),
                      (torch.tensor([0.0, 20.0]), "integer")):
        with pytest.raises(ValueError, match=word):
            pj.polyfilter_tod(tod, bad, 2)
    with pytest.raises(ValueError, match="order must be 0 to 7"):
        pj.polyfilter_tod(tod, [0, 50], 8)
    with pytest.raises(ValueError, match=r"rcond_min must lie in \[0, 1\)"):
        pj.polyfilter_tod(tod, [0, 50], 2, rcond_min=1.0)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        pj.polyfilter_tod(tod, [0, 25, 50], 2)                                  # a good seg_start: the next check is the device's


# ---- the filter-and-bin case on the numpy composition ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fb(pj, O):
    return FB.Case(pj, O)


def test_filter_bin_case_masked_recovers_the_source(fb):
    """With the mask on the source the fitted samples hold the drift alone, which the filter annihilates: the map is the sky, source
    included, to the rounding of a 10^3 drift.  Every pixel of the patch is solved, so no test of the case passes by cutting pixels."""
    m, solved, filt = fb.yardstick(True)
    on, off = fb.errors(m, solved)
    print("masked: solved %d of %d, error on the source %.3g, off it %.3g" % (solved.sum(), solved.size, on, off))
    assert solved.all()
    assert max(on, off) <= 1e-9                       # 10^3 x 2^-52 x the conditioning of a cubic fit and a 3 x 3 block: ~1e-12


def test_filter_bin_case_unmasked_biases_the_source(fb):
    """Without the mask the fit takes part of the source away: every source pixel's I is low by more than 10 % -- the evidence that
    the mask matters."""
    m, solved, _filt = fb.yardstick(False)
    bias = (fb.m0[0] - m[0])[fb.src] / FB.SRC_IQU[0]
    print("unmasked: the source's I is low by", bias)
    assert solved.all() and (bias > 0.10).all()
