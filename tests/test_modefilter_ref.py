"""tests/modefilter_ref.py, the yardstick of the detector-mode filter, held to the properties of the projection it
defines, and the parts of the feature that need no device: the refusals of the C entry and of the Python wrappers, the public
surface, and the mode-filter-and-bin case on the numpy composition.  CPU only.

The refusal calls pass HOST buffers to the raw library: they are made only where pxl_device_count() is 0, so that a wrongly
accepted call can never launch (tests/test_abi_point_args.py's rule)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
from host_arena import lib, mutated

import modefilter_case as MC
import modefilter_ref as MF
import polyfilter_ref as PF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PXL_EINVAL, PXL_EHIP = -22, -5
EPS = 2.0 ** -52


def _modes(rng, nd, K):
    """Ones, then couplings of order one: a common mode and K - 1 further array modes."""
    return np.concatenate([np.ones((nd, 1)), rng.normal(size=(nd, K - 1))], axis=1)


def _weights(kind, shape, rng):
    return None if kind == "uniform" else rng.uniform(0.25, 4.0, shape)


# ---- the yardstick's own properties -----------------------------------------------------------------------------------------------

def test_the_vector_solve_is_polyfilter_refs_solve():
    """modefilter_ref.solve over 60 columns gives polyfilter_ref.solve's bits column by column, full rank, rank lost at the first
    pivot and rank lost at the last."""
    rng = np.random.default_rng(2)
    K, T = 4, 60
    A = rng.normal(size=(K, 6, T))
    G = np.einsum("ikt,jkt->ijt", A, A)
    G[:, :, 10:20] = 0.0
    G[3, :, 20:30] = G[2, :, 20:30]
    G[:, 3, 20:30] = G[:, 2, 20:30]
    G[3, 3, 20:30] = G[2, 2, 20:30]                                             # mode 3 = mode 2: the last pivot is 0
    b = rng.normal(size=(K, T))
    for dtype in (np.float64, np.longdouble):
        c, nu, ratios = MF.solve(G.astype(dtype), b.astype(dtype), 1e-10, dtype)
        assert sorted(set(nu)) == [0, 3, 4]
        for t in range(T):
            c1, nu1, r1 = PF.solve(G[:, :, t].astype(dtype), b[:, t].astype(dtype), 1e-10, dtype)
            assert nu1 == nu[t] and np.array_equal(c1, c[:, t]) and np.array_equal(r1, ratios[:, t], equal_nan=True)


@pytest.mark.parametrize("kind", ["uniform", "random"])
@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_it_annihilates_a_timestream_of_its_modes(kind, dtype):
    """d = F c(t) group by group: out is rounding in every group, and the detectors outside the groups are copied.  The bound is
    polyfilter's: 100 eps / (the smallest accepted pivot ratio) max|d|."""
    rng = np.random.default_rng(5)
    nd, nt, grp = 40, 33, [2, 3, 12, 12, 37]
    for K in (1, 3, 8):
        F = _modes(rng, nd, K)
        d = np.zeros((nd, nt))
        for lo, hi in MF.clamp_groups(grp, nd):
            d[lo:hi] = F[lo:hi] @ rng.normal(size=(K, nt))
        d[:2], d[37:] = rng.normal(size=(2, nt)), rng.normal(size=(3, nt))
        fit = MF.filter(d, F, grp, wfit=_weights(kind, d.shape, rng), dtype=dtype)
        assert (fit.n_used[[1, 3]] == K).all() and (fit.n_used[0] == 1).all() and (fit.n_used[2] == 0).all()
        rmin = float(np.nanmin(np.asarray(fit.ratios[[1, 3]], dtype=np.float64)))
        out = np.asarray(fit.out, dtype=np.float64)
        resid = np.abs(out[2:37]).max()
        print("K = %d: smallest pivot ratio %.3g, residual %.3g of max|d| %.3g" % (K, rmin, resid, np.abs(d).max()))
        assert rmin > 1e-7 and resid <= 100 * EPS / rmin * np.abs(d).max()
        assert np.array_equal(out[:2], d[:2]) and np.array_equal(out[37:], d[37:])


@pytest.mark.parametrize("kind", ["uniform", "random"])
def test_it_is_idempotent(kind):
    """Z Z d = Z d: the second application changes a sample by rounding of the first's size."""
    rng = np.random.default_rng(6)
    nd, nt, grp = 30, 20, [0, 9, 30]
    d = rng.normal(size=(nd, nt))
    w = _weights(kind, d.shape, rng)
    for K in (1, 3, 6):
        F = _modes(rng, nd, K)
        once = MF.filter(d, F, grp, wfit=w).out
        twice = MF.filter(once, F, grp, wfit=w)
        print("K = %d: |ZZd - Zd| max %.3g, second amplitudes max %.3g" % (K, np.abs(twice.out - once).max(), np.abs(twice.amps).max()))
        assert np.abs(twice.out - once).max() <= 1e4 * EPS * np.abs(d).max()
        assert np.abs(twice.amps).max() <= 1e4 * EPS * np.abs(d).max()


@pytest.mark.parametrize("kind", ["uniform", "random"])
def test_it_is_the_dense_projector_per_column(kind):
    """One group of 12 detectors, K = 3, a weight vector of its own for each of 12 columns: column t of the filter applied to the
    identity is column t of Z_t = I - F (F^T W_t F)^-1 F^T W_t, and W_t Z_t is symmetric."""
    rng = np.random.default_rng(7)
    n, K = 12, 3
    F = _modes(rng, n, K)
    w = np.ones((n, n)) if kind == "uniform" else rng.uniform(0.25, 4.0, (n, n))
    out = MF.filter(np.eye(n), F, wfit=w).out                                    # column t: Z_t e_t
    for t in range(n):
        Z = MF.projector(F, w[:, t])
        WZ = w[:, t][:, None] * Z
        assert np.abs(out[:, t] - Z[:, t]).max() <= 1e-12 and np.abs(WZ - WZ.T).max() <= 1e-12 and np.abs(Z @ Z - Z).max() <= 1e-12


def test_truncation_counts_the_live_detectors():
    """A column with n live detectors is fitted with min(n, K) modes, the rest +0.0, and with fewer live detectors than modes its
    live samples come out as rounding; with none it is copied, -0.0 and NaN included.  Every summation order agrees."""
    rng = np.random.default_rng(8)
    nd = 20
    for K in (1, 3, 8):
        nt = K + 3                                                               # column t has t live detectors
        F = _modes(rng, nd, K)
        d = rng.normal(size=(nd, nt))
        d[0, 0], d[1, 0] = -0.0, np.nan
        w = np.zeros((nd, nt))
        for t in range(nt):
            live = rng.choice(nd, size=t, replace=False)
            w[live, t] = rng.uniform(0.5, 2.0, t)
        for dtype, phases in ((np.float64, None), (np.longdouble, None), (np.float64, 4), (np.float64, 16)):
            fit = MF.filter(d, F, wfit=w, dtype=dtype, phases=phases)
            assert np.array_equal(fit.n_used[0], np.minimum(np.arange(nt), K)), (K, fit.n_used, fit.ratios)
            amps = np.asarray(fit.amps[0], dtype=np.float64)
            past = np.arange(K)[:, None] >= fit.n_used[0][None, :]
            assert not amps[past].any() and not np.signbit(amps[past]).any()
            out = np.asarray(fit.out, dtype=np.float64)
            assert np.array_equal(out[:, 0].view(np.int64), d[:, 0].view(np.int64))
            for t in range(1, K + 1):                                            # t modes interpolate t live detectors
                r = np.asarray(fit.ratios[0, :t, t], dtype=np.float64)
                assert r.min() > 1e-10
                assert np.abs(out[w[:, t] > 0, t]).max() <= 100 * EPS / r.min() * np.abs(amps[:, t]).sum() * np.abs(F).max()


def test_the_tile_rule_reaches_both_sizes():
    assert MF.tile(1, 1) == 16 and MF.tile(64 * 511, 1) == 16 and MF.tile(64 * 511 + 1, 1) == 64 and MF.tile(100000, 1) == 64
    assert MF.tile(1, 511) == 16 and MF.tile(1, 512) == 64 and MF.tile(65, 256) == 64 and MF.tile(64, 256) == 16 and MF.tile(1000, 0) == 16


# ---- the C entry's refusals -------------------------------------------------------------------------------------------------------

ND, NT, NGRP, NMODES = 6, 40, 3, 2


SLOTS = ("grp_start", "modes", "d", "wfit", "out", "amps", "n_used")


def _entry(lib, v):
    return lib.pxl_tod_modefilter_f64(v["n_det"], v["n_t"], v["n_grp"], v["grp_start"], v["n_modes"], v["modes"], v["rcond_min"], v["d"],
                                      v["wfit"], v["out"], v["amps"], v["n_used"], None)


_mutated = functools.partial(mutated, SLOTS, dict(n_det=ND, n_t=NT, n_grp=NGRP, n_modes=NMODES, rcond_min=1e-10), _entry)


REFUSALS = [
    ("n_modes_zero", dict(n_modes=0), "n_modes"),
    ("n_modes_negative", dict(n_modes=-1), "n_modes"),
    ("n_modes_nine", dict(n_modes=9), "n_modes"),
    ("rcond_min_negative", dict(rcond_min=-1e-3), "rcond_min"),
    ("rcond_min_one", dict(rcond_min=1.0), "rcond_min"),
    ("rcond_min_nan", dict(rcond_min=float("nan")), "rcond_min"),
    ("n_det_negative", dict(n_det=-1), "n_det"),
    ("n_t_negative", dict(n_t=-1), "n_t"),
    ("n_grp_negative", dict(n_grp=-1), "n_grp"),
    ("n_overflows", dict(n_det=2 ** 40, n_t=2 ** 40), "n_det * n_t"),
    ("bytes_overflow", dict(n_det=2 ** 30, n_t=2 ** 30), "n_det * n_t"),
    ("modes_bytes_overflow", dict(n_det=2 ** 59, n_t=1, n_modes=8), "n_det * n_modes"),
    ("groups_overflow", dict(n_t=2 ** 31, n_grp=2 ** 40), "n_grp * n_t"),
    ("amps_bytes_overflow", dict(n_t=2 ** 29, n_grp=2 ** 29, n_modes=8), "n_grp * n_t"),
    ("grp_bytes_overflow", dict(n_t=1, n_grp=2 ** 62), "n_grp * n_t"),
    ("d_null", dict(d=None), "null d"),
    ("out_null", dict(out=None), "null out"),
    ("grp_start_null", dict(grp_start=None), "null grp_start"),
    ("modes_null", dict(modes=None), "null modes"),
    ("d_misaligned", dict(d="@d+4"), "8-byte aligned"),
    ("modes_misaligned", dict(modes="@modes+4"), "8-byte aligned"),
    ("out_shifted_on_d", dict(out="@d+8"), "out overlaps d other than exactly"),
    ("out_on_wfit", dict(out="@wfit"), "out overlaps wfit"),
    ("out_on_grp_start", dict(out="@grp_start"), "out overlaps grp_start"),
    ("out_on_modes", dict(out="@modes+8"), "out overlaps modes"),
    ("amps_on_d", dict(amps="@d"), "amps overlaps d"),
    ("amps_on_wfit", dict(amps="@wfit+64"), "amps overlaps wfit"),
    ("amps_on_grp_start", dict(amps="@grp_start"), "amps overlaps grp_start"),
    ("amps_on_modes", dict(amps="@modes"), "amps overlaps modes"),
    ("amps_on_out", dict(amps="@out"), "amps overlaps out"),
    ("n_used_on_d", dict(n_used="@d+16"), "n_used overlaps d"),
    ("n_used_on_wfit", dict(n_used="@wfit"), "n_used overlaps wfit"),
    ("n_used_on_grp_start", dict(n_used="@grp_start+8"), "n_used overlaps grp_start"),
    ("n_used_on_modes", dict(n_used="@modes"), "n_used overlaps modes"),
    ("n_used_on_out", dict(n_used="@out"), "n_used overlaps out"),
    ("n_used_on_amps", dict(n_used="@amps+8"), "n_used overlaps amps"),
    ("amps_on_d_in_place", dict(out="@d", amps="@d"), "amps overlaps"),
    # 3 * 2^30 and 2^31 + 2 blocks (past 2^31 - 1 the tile is always the wide one); the buffers are 2^39 and 2^34 bytes, so in place,
    # without the optional ones, and with grp_start far from the arena
    ("too_many_tiles", dict(n_det=1, n_t=2 ** 36, n_grp=1, out="@d", wfit=None, amps=None, n_used=None), "blocks"),
    ("too_many_groups", dict(n_det=1, n_t=64, n_grp=2 ** 31, grp_start=2 ** 50, amps=None, n_used=None), "blocks"),
]


def test_the_entry_refuses_with_a_text_that_names_the_argument(pj, lib):
    wrong = {}
    for name, changes, word in REFUSALS:
        rc, text = _mutated(**changes).call(pj, lib)
        if rc != PXL_EINVAL or word not in text or not text.startswith("tod_modefilter"):
            wrong[name] = (rc, text)
    assert not wrong, wrong


def test_valid_and_empty_calls(pj, lib):
    """A call that passes every check reaches its kernel (PXL_EHIP: there is no device); every allowed null and the in-place form
    are accepted, at every number of modes; a call with no samples returns 0 before that, whatever else it holds."""
    valid = [dict(), dict(wfit=None), dict(amps=None), dict(n_used=None), dict(out="@d"), dict(n_grp=0), dict(rcond_min=0.0)]
    for changes in valid + [dict(n_modes=k) for k in range(1, 9)]:
        rc, text = _mutated(**changes).call(pj, lib)
        assert rc == PXL_EHIP and text.startswith("launch of k_modefilter"), (changes, rc, text)
    for changes in (dict(n_det=0), dict(n_t=0), dict(n_det=0, d=None, out=None, grp_start=None, modes=None), dict(n_t=0, out="@wfit")):
        assert _mutated(**changes).call(pj, lib) == (0, ""), changes


# ---- the surface ------------------------------------------------------------------------------------------------------------------------

def test_the_new_names_are_exported_and_bound(pj):
    for name in ("modefilter_tod", "common_mode_tod", "filter_bin_map_pol_nearest_tod"):
        assert callable(getattr(pj, name))
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/pixell_hip.h").read(), flags=re.S)
    julia = open(ROOT + "/julia/PixellHIP.jl").read()
    name = "pxl_tod_modefilter_f64"
    assert name in header and name in pj._lib.SIGNATURES and ":" + name in julia
    sig = pj._lib.SIGNATURES[name][1]
    assert len(sig) == 13 and sig[4] is C.c_int and sig[6] is C.c_double
    assert "function modefilter!" in julia and re.search(r"^export .*\bmodefilter!", julia, flags=re.M)
    assert '@testset "modefilter!' in open(ROOT + "/julia/test_pixellhip.jl").read()
    import inspect
    p = inspect.signature(pj.filter_bin_map_pol_nearest_tod).parameters
    assert list(p)[-4:] == ["chunk_t", "modes", "grp_start", "mode_rcond_min"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("modes", "grp_start", "mode_rcond_min"))
    assert p["modes"].default is None and p["grp_start"].default is None and p["mode_rcond_min"].default == 1e-10


def test_the_wrappers_refuse_on_the_host_before_they_need_a_device(pj):
    """grp_start is checked on the host, before the device checks: decreasing, below 0, past D, empty, not integers."""
    import torch
    tod = torch.zeros((6, 50), dtype=torch.float64)
    F = torch.ones((6, 2), dtype=torch.float64)
    for bad, word in (([0, 4, 3, 6], "non-decreasing"), ([-1, 3, 6], r"inside \[0, D\]"), ([0, 3, 7], r"inside \[0, D\]"),
                      (torch.tensor([5, 2]), "non-decreasing"), ([], "at least one"), ([0.5, 3], "integers"),
                      (torch.tensor([0.0, 3.0]), "integer")):
        with pytest.raises(ValueError, match=word):
            pj.modefilter_tod(tod, F, grp_start=bad)
        with pytest.raises(ValueError, match="common_mode_tod: grp_start"):
            pj.common_mode_tod(tod, grp_start=bad)
    with pytest.raises(ValueError, match=r"modes is a \(D, K\)"):
        pj.modefilter_tod(tod, torch.ones((5, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="1 to 8 modes"):
        pj.modefilter_tod(tod, torch.ones((6, 9), dtype=torch.float64))
    with pytest.raises(ValueError, match="1 to 8 modes"):
        pj.modefilter_tod(tod, torch.ones((6, 0), dtype=torch.float64))
    with pytest.raises(ValueError, match="Float64 modes"):
        pj.modefilter_tod(tod, F.float())
    with pytest.raises(ValueError, match=r"rcond_min must lie in \[0, 1\)"):
        pj.modefilter_tod(tod, F, rcond_min=1.0)
    with pytest.raises(ValueError, match=r"gains is a \(D,\)"):
        pj.common_mode_tod(tod, gains=F)
    with pytest.raises(ValueError, match=r"tod is a \(D, T\)"):
        pj.common_mode_tod(tod[0])
    for call in (lambda: pj.modefilter_tod(tod, F, grp_start=[0, 3, 6]), lambda: pj.modefilter_tod(tod, F[:, 0]), lambda: pj.common_mode_tod(tod)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):       # good host arguments: the next check is the device's
            call()


# ---- the mode-filter-and-bin case on the numpy composition ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mc(pj, O):
    return MC.Case(pj, O)


def test_mode_bin_case_filtered_recovers_the_sky(mc):
    """With the source masked the live detectors hold the common signal alone, which the filter annihilates in every detector: the
    map is the sky, source included, to the rounding of a 10^3 signal.  Every pixel of the patch is solved."""
    m, solved, _filt = mc.yardstick(True)
    on, off = mc.errors(m, solved)
    print("filtered: solved %d of %d, error on the source %.3g, off it %.3g" % (solved.sum(), solved.size, on, off))
    assert solved.all()
    assert max(on, off) <= 1e-10                      # 10^3 x 2^-52 x a few detectors and hits: ~1e-13


def test_mode_bin_case_unfiltered_is_wrong_by_more_than_the_source(mc):
    """Without the mode filter the common signal goes into the map, with or without a mean taken off every detector and sweep:
    the worst pixel is wrong by more than the source's amplitude."""
    m, solved, _filt = mc.yardstick(False)
    assert solved.all() and max(mc.errors(m, solved)) > MC.SRC_IQU[0]
    poly = PF.filter(mc.tod, mc.seg_start, MC.POLY_ORDER, wfit=mc.w_fit(True)).out
    m, solved = mc.bin(poly)
    print("unfiltered: worst error on and off the source", mc.errors(m, solved))
    assert solved.all() and max(mc.errors(m, solved)) > MC.SRC_IQU[0]
