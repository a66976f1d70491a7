"""tests/binfilter_ref.py, the yardstick of the binned-template filter, held to the properties of the projection it
defines and to the polynomial filter's yardstick at order 0, and the parts of the feature that need no device: pj.bin_plan and
pj.scan_bins (torch on the host), the refusals of the C entry and of the Python wrapper, the public surface, the template-and-bin
case on the numpy composition, and the cap on the inputs that the device test sets aside from its accuracy bar.  CPU only.

The refusal calls pass HOST buffers to the raw library: they are made only where pxl_device_count() is 0, so that a wrongly
accepted call can never launch (tests/test_abi_point_args.py's rule)."""
import functools
import os
import re

import numpy as np
import pytest
import torch
from host_arena import lib, mutated

import binfilter_case as BC
import binfilter_layouts as BL
import binfilter_ref as BF
import fit_ref
import polyfilter_ref as PF
from conftest import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PXL_EINVAL, PXL_EHIP = -22, -5
EPS = 2.0 ** -52


def _weights(kind, shape, rng):
    return None if kind == "uniform" else rng.uniform(0.25, 4.0, shape)


# ---- the yardstick's own properties -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["uniform", "random"])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_it_annihilates_every_signal_that_is_constant_on_bins(kind, dtype):
    """d = one constant per (detector, bin): out is rounding in every bin -- a mean of n equal values of size a is a within n eps a
    -- and the samples in no bin are copied."""
    rng = np.random.default_rng(5)
    nt, n_bin = 400, 7
    index = BL.triangle(nt, n_bin, 90, turn=0.04)
    order, bin_start = BF.plan(index, n_bin)
    level = rng.normal(size=(2, n_bin)) * 100.0
    d = np.where(index >= 0, level[:, np.maximum(index, 0)], rng.normal(size=(2, nt)))
    fit = BF.filter(d, order, bin_start, wfit=_weights(kind, d.shape, rng), dtype=dtype)
    out = np.asarray(fit.out, dtype=np.float64)
    print("residual %.3g of max|d| %.3g" % (np.abs(out[:, index >= 0]).max(), np.abs(d).max()))
    assert (fit.n_used == 1).all() and (index < 0).any()
    assert np.abs(out[:, index >= 0]).max() <= nt * EPS * np.abs(d).max()
    assert np.abs(np.asarray(fit.means, dtype=np.float64) - level).max() <= nt * EPS * np.abs(d).max()
    assert np.array_equal(out[:, index < 0], d[:, index < 0])


@pytest.mark.parametrize("kind", ["uniform", "random"])
def test_it_is_idempotent(kind):
    """Z Z d = Z d: the second application changes a sample by rounding of the first's size."""
    rng = np.random.default_rng(6)
    order, bin_start = BF.plan(rng.integers(-1, 9, 400), 9)
    d = rng.normal(size=(2, 400))
    w = _weights(kind, d.shape, rng)
    once = BF.filter(d, order, bin_start, wfit=w).out
    twice = BF.filter(once, order, bin_start, wfit=w)
    print("|ZZd - Zd| max %.3g, second means max %.3g" % (np.abs(twice.out - once).max(), np.abs(twice.means).max()))
    assert np.abs(twice.out - once).max() <= 1e3 * EPS * np.abs(d).max()
    assert np.abs(twice.means).max() <= 1e3 * EPS * np.abs(d).max()


@pytest.mark.parametrize("kind", ["uniform", "random"])
def test_wz_is_symmetric_and_the_filter_is_the_dense_projector(kind):
    """12 samples in 3 bins that interleave in time: the columns of the filter are Z = I - F (F^T W F)^-1 F^T W with F the bins'
    indicator, and W Z is symmetric."""
    rng = np.random.default_rng(7)
    n, n_bin = 12, 3
    index = rng.permutation(np.arange(n) % n_bin)
    order, bin_start = BF.plan(index, n_bin)
    w = np.ones(n) if kind == "uniform" else rng.uniform(0.25, 4.0, n)
    Z = np.stack([BF.filter(np.eye(n)[i][None], order, bin_start, wfit=w[None]).out[0] for i in range(n)], axis=1)
    dense = fit_ref.projector(index[:, None] == np.arange(n_bin)[None, :], w)
    WZ = w[:, None] * Z
    print("|Z - dense| max %.3g, asymmetry of W Z %.3g" % (np.abs(Z - dense).max(), np.abs(WZ - WZ.T).max()))
    assert np.abs(Z - dense).max() <= 1e-12 and np.abs(WZ - WZ.T).max() <= 1e-12
    assert np.abs(Z @ Z - Z).max() <= 1e-12


@pytest.mark.parametrize("nd,nt,seg", [(3, 130, [2, 3, 5, 68, 68, 130]), (2, 1100, [38, 1062]), (1, 5000, [0, 5000]), (3, 130, list(range(0, 131, 2)))])
def test_contiguous_bins_are_the_polynomial_yardstick_at_order_zero_by_bits(nd, nt, seg):
    """With an identity order and bins that are segments the two yardsticks, independent transcriptions, give the same bits: out,
    the mean against the coefficient, n_used -- sequentially and in the device's order, whose G is the same."""
    d, w = BL.make_data(nd, nt, 11 + nt)
    ident = np.arange(nt)
    G = BF.group(nt, len(seg) - 1)
    assert G == PF.group(nt, len(seg) - 1, 0)
    for lanes in (None, G):
        mine = BF.filter(d, ident, seg, wfit=w, lanes=lanes)
        poly = PF.filter(d, seg, 0, wfit=w, rcond_min=0.0, lanes=lanes)
        assert bits_equal(mine.out, poly.out) and bits_equal(mine.means, poly.coeffs[:, :, 0]) and np.array_equal(mine.n_used, poly.n_used)


def test_truncation_a_bin_without_a_positive_finite_weight_sum_is_copied():
    """0 live samples and an infinite sum of weights: n_used = 0, the mean +0.0, the bits of d, -0.0 and NaN included; 1 live sample:
    n_used = 1 and that sample comes out +0.0."""
    rng = np.random.default_rng(8)
    L = 40
    d = rng.normal(size=(3, L))
    d[:, 0], d[:, 1] = -0.0, np.nan
    w = np.zeros((3, L))
    w[1, 7] = 1.5
    w[2, 5], w[2, 9] = np.inf, 1.0
    for dtype in (np.float64, np.longdouble):
        fit = BF.filter(d, np.arange(L), [0, L], wfit=w, dtype=dtype)
        out = np.asarray(fit.out, dtype=np.float64)
        assert fit.n_used[:, 0].tolist() == [0, 1, 0] and not np.signbit(np.asarray(fit.means, dtype=np.float64)).any()
        assert fit.means[0, 0] == 0 and fit.means[2, 0] == 0 and fit.means[1, 0] == d[1, 7]
        assert np.array_equal(out[[0, 2]].view(np.int64), d[[0, 2]].view(np.int64))
        assert out[1, 7] == 0.0 and np.isnan(out[1, 1])


def test_the_group_rule_is_the_polynomial_filters_at_order_zero():
    assert all(BF.group(nt, nb) == PF.group(nt, nb, 0) for nt in (1, 130, 1100, 5000, 10 ** 5) for nb in range(0, 300))
    assert BF.group(5000, 4) == 256 and BF.group(1, 1) == 1 and BF.group(10 ** 5, 200) == 64


def test_the_layouts_reach_every_group_size_length_and_kind_of_plan():
    lays = BL.layouts()
    assert {(nd, nt) for _n, nd, nt, _o, _b in lays} == {(1, 1), (3, 130), (2, 1100), (1, 5000)}
    assert {BF.group(nt, len(b) - 1) for _n, _nd, nt, _o, b in lays} == {1, 2, 4, 8, 16, 32, 64, 256}
    lengths = {hi - lo for _n, _nd, nt, _o, b in lays for lo, hi in fit_ref.clamp(b, nt)}
    assert {0, 1, 2, 63, 64, 65, 257, 1023, 1024, 5000} <= lengths
    trips = {-(-(hi - lo) // BF.group(nt, len(b) - 1)) for _n, _nd, nt, _o, b in lays for lo, hi in fit_ref.clamp(b, nt)}
    assert {1, 2, 5, 14, 16, 20} <= trips and max(trips) == 20
    assert any(b[0] > 0 for _n, _nd, _nt, _o, b in lays) and any(b[-1] < nt for _n, _nd, nt, _o, b in lays)
    assert any((np.diff(b) == 0).all() for _n, _nd, _nt, _o, b in lays)                      # every sample out of range
    for _n, _nd, nt, order, b in lays:                                                         # every one a valid plan
        assert np.array_equal(np.sort(order), np.arange(nt)) and (np.diff(b) >= 0).all() and b[0] >= 0 and b[-1] <= nt
    # the scans stay 1 to 20 consecutive samples in a bin
    runs = set()
    for period, n_bin in ((130, 65), (64, 16), (48, 8), (52, 4), (400, 40), (160, 4), (2000, 200)):
        k = BL.triangle(4 * period, n_bin, period)
        edges = np.flatnonzero(np.diff(k) != 0)
        runs |= set(np.diff(edges).tolist())
    assert min(runs) == 1 and max(runs) <= 40 and 20 in runs and 5 in runs


def test_at_most_one_layout_in_ten_is_set_aside():
    """The cap of tests/binfilter_layouts.py on the committed seeds, decided by the yardstick alone."""
    lays = BL.layouts()
    aside = [lays[k][0] for k in range(len(lays)) if not BL.case(k).admitted]
    worst = max(BL.case(k).clause(BL.case(k).lanes)[1] for k in range(len(lays)))
    print("set aside from the accuracy bar: %d of %d %s; the device's order in numpy is at worst %.3f of the bar" % (len(aside), len(lays), aside, worst))
    assert 10 * len(aside) <= len(lays)


# ---- bin_plan and scan_bins ---------------------------------------------------------------------------------------------------------

def test_bin_plan_is_stable_counts_and_equals_the_numpy_plan(pj):
    rng = np.random.default_rng(12)
    for n_bin, index in ((5, rng.integers(-3, 9, 300)), (1, np.zeros(7, dtype=np.int64)), (4, np.full(20, -1)), (3, np.zeros(0, dtype=np.int64)),
                         (200, BL.triangle(5000, 200, 2000, turn=0.01))):
        for arg in (index, torch.from_numpy(index), torch.from_numpy(index).to(torch.int32)):
            order, bin_start = pj.bin_plan(arg, n_bin)
            assert order.dtype == torch.int64 and bin_start.dtype == torch.int64 and bin_start.shape == (n_bin + 1,)
            order, bin_start = order.numpy(), bin_start.numpy()
            ref_order, ref_start = BF.plan(index, n_bin)
            assert np.array_equal(order, ref_order) and np.array_equal(bin_start, ref_start)
            ok = (index >= 0) & (index < n_bin)
            for b in range(n_bin):
                assert np.array_equal(order[bin_start[b]:bin_start[b + 1]], np.flatnonzero(index == b))        # time order inside the bin
            assert np.array_equal(order[bin_start[n_bin]:], np.flatnonzero(~ok)) and bin_start[0] == 0         # the unfiltered samples last
            assert bin_start[n_bin] == ok.sum()
    with pytest.raises(ValueError, match="n_bin must be at least 1"):
        pj.bin_plan(np.zeros(4, dtype=np.int64), 0)
    for bad in (np.zeros(4), torch.zeros(4), np.zeros((2, 2), dtype=np.int64), np.zeros(4, dtype=bool)):
        with pytest.raises(ValueError, match="integers"):
            pj.bin_plan(bad, 3)


def test_scan_bins_on_a_triangle_wave(pj):
    """az sweeps 10 -> 30 -> 10 in steps of 0.5, binned into 8 bins on [12, 28): the edges fall on samples, the ends are -1, the way
    back is split off, and a NaN is -1."""
    up = 10.0 + 0.5 * np.arange(41)
    az = np.concatenate([up, up[-2::-1], up[1:]])
    k = pj.scan_bins(az, 8, 12.0, 28.0).numpy()
    want = np.where((az >= 12.0) & (az < 28.0), np.floor((az - 12.0) / 2.0), -1).astype(np.int64)
    assert k.dtype == np.int64 and np.array_equal(k, want)
    assert k[4] == 0 and k[3] == -1 and k[35] == 7 and k[36] == -1 and k[7] == 0 and k[8] == 1  # 12.0 is in, 28.0 is out, 14.0 opens bin 1
    split = pj.scan_bins(torch.from_numpy(az), 8, 12.0, 28.0, split_direction=True).numpy()
    back = np.zeros(len(az), dtype=bool)
    back[41:80] = True                                                                          # the samples between the two turning points
    assert np.array_equal(split, np.where(want >= 0, want + 8 * back, -1))
    assert not back[40] and not back[80]                                                        # at a turning point the central difference is 0: forward
    bad = az.copy()
    bad[10], bad[11] = np.nan, np.nan
    kb = pj.scan_bins(bad, 8, 12.0, 28.0, split_direction=True).numpy()
    assert kb[10] == -1 and kb[11] == -1 and kb[9] == want[9] and kb[12] == want[12]            # a NaN neighbour's difference is not negative
    assert pj.scan_bins(np.array([np.inf, -np.inf, 13.0]), 8, 12.0, 28.0).numpy().tolist() == [-1, -1, 0]
    assert pj.scan_bins(np.array([np.nextafter(28.0, 0.0)]), 3, 12.0, 28.0).numpy()[0] == 2    # just below hi: the last bin, never n_bin
    for args in ((az, 0, 0.0, 1.0), (az, 4, 1.0, 1.0), (az, 4, 0.0, np.inf), (az.astype(np.float32), 4, 0.0, 1.0)):
        with pytest.raises(ValueError):
            pj.scan_bins(*args)


# ---- the C entry's refusals -------------------------------------------------------------------------------------------------------

ND, NT, NBIN = 3, 40, 4
SLOTS = ("bin_start", "order", "d", "wfit", "out", "means", "n_used")


def _entry(lib, v):
    return lib.pxl_tod_binfilter_f64(v["n_det"], v["n_t"], v["n_bin"], v["bin_start"], v["order"], v["d"], v["wfit"], v["out"], v["means"],
                                     v["n_used"], None)


_mutated = functools.partial(mutated, SLOTS, dict(n_det=ND, n_t=NT, n_bin=NBIN), _entry)

REFUSALS = [
    ("n_det_negative", dict(n_det=-1), "n_det"),
    ("n_t_negative", dict(n_t=-1), "n_t"),
    ("n_bin_negative", dict(n_bin=-1), "n_bin"),
    ("n_overflows", dict(n_det=2 ** 40, n_t=2 ** 40), "n_det * n_t"),
    ("bytes_overflow", dict(n_det=2 ** 30, n_t=2 ** 30), "n_det * n_t"),
    ("bins_overflow", dict(n_det=2 ** 31, n_bin=2 ** 40), "n_det * n_bin"),
    ("mean_bytes_overflow", dict(n_det=2 ** 30, n_bin=2 ** 30), "n_det * n_bin"),
    ("bin_bytes_overflow", dict(n_det=1, n_bin=2 ** 62), "n_det * n_bin"),
    ("blocks_overflow", dict(n_det=2 ** 31, n_t=32, n_bin=510, out="@d", wfit=None, means=None, n_used=None), "too large for one launch"),
    ("d_null", dict(d=None), "null d"),
    ("out_null", dict(out=None), "null out"),
    ("bin_start_null", dict(bin_start=None), "null bin_start"),
    ("order_null", dict(order=None), "null order"),
    ("d_misaligned", dict(d="@d+4"), "8-byte aligned"),
    ("order_misaligned", dict(order="@order+4"), "8-byte aligned"),
    ("out_shifted_on_d", dict(out="@d+8"), "out overlaps d other than exactly"),
    ("out_on_wfit", dict(out="@wfit"), "out overlaps wfit"),
    ("out_on_bin_start", dict(out="@bin_start"), "out overlaps bin_start"),
    ("out_on_order", dict(out="@order"), "out overlaps order"),
    ("means_on_d", dict(means="@d"), "means overlaps d"),
    ("means_on_wfit", dict(means="@wfit+64"), "means overlaps wfit"),
    ("means_on_bin_start", dict(means="@bin_start"), "means overlaps bin_start"),
    ("means_on_order", dict(means="@order+8"), "means overlaps order"),
    ("means_on_out", dict(means="@out"), "means overlaps out"),
    ("n_used_on_d", dict(n_used="@d+16"), "n_used overlaps d"),
    ("n_used_on_order", dict(n_used="@order"), "n_used overlaps order"),
    ("n_used_on_out", dict(n_used="@out"), "n_used overlaps out"),
    ("n_used_on_means", dict(n_used="@means+8"), "n_used overlaps means"),
    ("means_on_d_in_place", dict(out="@d", means="@d"), "means overlaps"),
]


def test_the_entry_refuses_with_a_text_that_names_the_argument(pj, lib):
    wrong = {}
    for name, changes, word in REFUSALS:
        rc, text = _mutated(**changes).call(pj, lib)
        if rc != PXL_EINVAL or word not in text or not text.startswith("tod_binfilter"):
            wrong[name] = (rc, text)
    assert not wrong, wrong


def test_valid_and_empty_calls(pj, lib):
    """A call that passes every check reaches its kernel (PXL_EHIP: there is no device); every allowed null and the in-place form
    are accepted; a call with no samples returns 0 before that, whatever else it holds."""
    for changes in (dict(), dict(wfit=None), dict(means=None), dict(n_used=None), dict(means=None, n_used=None), dict(out="@d"), dict(n_bin=0)):
        rc, text = _mutated(**changes).call(pj, lib)
        assert rc == PXL_EHIP and text.startswith("launch of k_binfilter"), (changes, rc, text)
    for changes in (dict(n_det=0), dict(n_t=0), dict(n_det=0, d=None, out=None, bin_start=None, order=None), dict(n_t=0, out="@wfit", order=None)):
        assert _mutated(**changes).call(pj, lib) == (0, ""), changes


# ---- the surface ------------------------------------------------------------------------------------------------------------------------

def test_the_new_names_are_exported_and_bound(pj):
    for name in ("binfilter_tod", "bin_plan", "scan_bins", "template_bin_map_pol_nearest_tod"):
        assert callable(getattr(pj, name))
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pixell_hip.h").read(), flags=re.S)
    julia = open(ROOT + "/julia/PixellHIP.jl").read()
    name = "pxl_tod_binfilter_f64"
    assert name in header and name in pj._lib.SIGNATURES and ":" + name in julia
    assert len(pj._lib.SIGNATURES[name][1]) == 11
    for fn in ("binfilter!", "bin_plan"):
        assert "function " + fn in julia and re.search(r"^export .*\b" + re.escape(fn), julia, flags=re.M)
    assert '@testset "binfilter!' in open(ROOT + "/julia/test_pixellhip.jl").read()
    import inspect
    old, new = (list(inspect.signature(f).parameters) for f in (pj.filter_bin_map_pol_nearest_tod, pj.template_bin_map_pol_nearest_tod))
    assert "bins" not in old and new == old[:7] + ["bins"] + old[7:]                 # the map-maker's arguments, bins after the geometry
    p = inspect.signature(pj.template_bin_map_pol_nearest_tod).parameters
    assert p["seg_start"].default is None and p["order"].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("modes", "grp_start", "mode_rcond_min"))


def test_the_wrapper_refuses_a_bad_plan_before_it_needs_a_device(pj):
    """The plan is checked on the host, before the device checks: the wrong length, decreasing offsets, an offset beyond T, an order
    that is not a permutation, and what is no plan at all."""
    nt = 50
    tod = torch.zeros((2, nt), dtype=torch.float64)
    order, bin_start = pj.bin_plan(np.arange(nt) % 5, 5)
    t = lambda v: torch.tensor(v, dtype=torch.int64)
    twice = order.clone()
    twice[3] = twice[4]
    outside = order.clone()
    outside[0] = nt
    for bad, word in (((order[:-1], bin_start), "one entry per time sample"), ((order, t([0, 30, 20, 50])), "non-decreasing"),
                      ((order, t([0, 20, 51])), r"inside \[0, T\]"), ((order, t([-1, 20, 50])), r"inside \[0, T\]"),
                      ((twice, bin_start), "permutation"), ((outside, bin_start), "permutation"),
                      ((order.to(torch.int32), bin_start), "int64"), ((order, bin_start.double()), "int64"),
                      (order, "plan is the"), ((order, bin_start, bin_start), "plan is the"), ((order, t([])), "at least one")):
        with pytest.raises(ValueError, match=word):
            pj.binfilter_tod(tod, bad)
    with pytest.raises(ValueError, match="one entry per time sample"):
        pj.binfilter_tod(tod, np.arange(nt - 1) % 5, n_bin=5)
    with pytest.raises(ValueError, match="integers"):
        pj.binfilter_tod(tod, np.zeros(nt), n_bin=5)
    with pytest.raises(ValueError, match="n_bin must be at least 1"):
        pj.binfilter_tod(tod, np.arange(nt) % 5, n_bin=0)
    with pytest.raises(ValueError, match="Float64 tod"):
        pj.binfilter_tod(tod.float(), (order, bin_start))
    for plan, kw in (((order, bin_start), {}), (np.arange(nt) % 5, dict(n_bin=5))):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            pj.binfilter_tod(tod, plan, **kw)                                   # a good plan: the next check is the device's


# ---- the template-and-bin case on the numpy composition -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def bc(pj, O):
    return BC.Case(pj, O)


def test_binfilter_case_masked_recovers_the_source(bc):
    """With the mask on the source the fitted samples hold the pickup alone, which the filter annihilates: the map is the sky, source
    included, to the rounding of a 10^3 pickup.  Every pixel of the patch is solved."""
    m, solved, _filt = bc.yardstick(True)
    on, off = bc.errors(m, solved)
    print("masked: solved %d of %d, error on the source %.3g, off it %.3g" % (solved.sum(), solved.size, on, off))
    assert solved.all()
    assert max(on, off) <= 1e-10                      # 10^3 x 2^-52 x a mean of 48 samples and a 3 x 3 block: ~1e-12


def test_binfilter_case_unmasked_biases_the_source_and_unfiltered_is_wrong(bc):
    """Without the mask the means take part of the source away: every source pixel's I is low, by far more than the masked error --
    the evidence that the mask matters.  Without the filter the map is wrong by the order of the pickup."""
    m, solved, _filt = bc.yardstick(False)
    bias = (bc.m0[0] - m[0])[bc.src]
    print("unmasked: the source's I is low by", bias)
    assert solved.all() and (bias > 1e-3).all()
    raw, solved, _filt = bc.yardstick(False, filtered=False)
    assert solved.all() and max(bc.errors(raw, solved)) > 0.1 * BC.PICKUP
