"""What tests/large_tod_case.py claims, shown on the CPU (no device): the thresholds each case crosses and where, the odd period
and what a lost high bit would land on, the exact-input cases' independence of the number of copies, the two forms of the
Toeplitz expectation on long segments, and the plans' bytes and kernel paths."""
import numpy as np
import pytest

import binfilter_ref as BF
import large_tod_case as LT
import modefilter_ref as MF
import polyfilter_ref as PF
import toeplitz_ref as TR
from conftest import bits_equal

CASES = LT.all_cases()
IDS = [LT.case_id(b, a) for b, a in CASES]
MAIN = {"polyfilter": ("d", "w"), "binfilter": ("d", "w"), "modefilter": ("d", "w"), "toeplitz": ("x", "out"), "pointing": ("sky", "resp")}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_the_sizes_are_what_the_case_module_states():
    assert len(IDS) == len(set(IDS)) == 35
    assert LT.T_B % 64 and LT.T_B % 256 and LT.T_B % 1280 and LT.SLAB <= 2 ** 28
    for tier, thr in (("A", 2 ** 29), ("B", 2 ** 31)):
        n_det, k, n_t = LT.long_shape(tier)
        assert n_t > thr and n_det == (3 if tier == "A" else 2)
        past = n_det * LT.PAST if tier == "B" else 0                  # large_tod_case's docstring: why a tier-B row is longer
        assert LT.TOTAL[tier] + past + n_det * LT.T_B < n_det * n_t < LT.TOTAL[tier] + past + 4 * n_det * LT.T_B
        kw = LT.wide_k(tier)
        assert LT.TOTAL[tier] + LT.ROWS * LT.T_B < kw * LT.ROWS * LT.T_B <= LT.TOTAL[tier] + 2 * LT.ROWS * LT.T_B


# per big buffer: how many elements make one row of it (None: it is not laid out in rows of time samples)
def _row_len(c, name):
    if name in ("d", "w", "out", "x") or (c.op == "modefilter" and name in ("amps", "n_used")):
        return c.n_t                                                  # amps: a row per (group, mode); n_used: a row per group
    if name in ("sky", "resp"):
        return 2 * c.n_t                                              # Float64 values of a row of double2
    return None


@pytest.mark.parametrize("builder,args", CASES, ids=IDS)
def test_thresholds(builder, args):
    """min < threshold <= max for the flat offsets of EVERY big buffer of the case, inputs, outputs and plans alike, for every threshold
    its size reaches; the (D, T) buffers reach every threshold the tier names.  In a buffer laid out in rows of time samples the
    crossing element is no row's first or last sample, and in a (D, T) buffer no segment's or bin's first."""
    c = builder(*args)
    want = [2 ** 29, 2 ** 31] + ([2 ** 32] if c.tier == "B" else [])
    per_elem = 2 if c.op == "pointing" else 1                         # a double2 output: the thresholds count elements
    reached = {}
    for name, n in c.big.items():
        main = name in MAIN[c.op] or (name == "out" and not c.in_place)
        elems = n // (per_elem if name in ("sky", "resp") else 1)
        reached[name] = LT.crossings(elems)
        if main:
            assert n == per_elem * c.n_det * c.n_t and reached[name] == want, (name, reached[name])
        for th in reached[name]:
            assert 0 < th <= elems - 1                                # min offset 0 < threshold <= max offset
            row_len = _row_len(c, name)
            if row_len is None:
                continue
            row, t = divmod(th * (per_elem if name in ("sky", "resp") else 1), row_len)
            assert 0 < t < row_len - 1 and row < n // row_len, (name, th)
            if main:
                at = (t - c.lead) % LT.T_B if c.starts_tiled else t
                assert at not in c.starts, (name, th, row, t)
    assert all(name in reached for name in MAIN[c.op])
    if c.op == "modefilter" and c.tier == "A" and (c.shape == "L" or (c.shape == "W" and c.K == 3)):
        assert reached["amps"] == [2 ** 29] and (c.shape == "W" or reached["n_used"] == [2 ** 29])    # the fit's outputs that are big
    if c.op == "pointing":
        assert 16 * (c.n - 1) > 2 ** 32 and (c.n_det - 1) * c.n_t + c.n_t - 1 >= 2 ** 31
        if c.shape == "L":
            assert 16 * c.n_t > 2 ** 32                               # byte offsets pass 2^32 inside the first row
    if c.shape == "L" and c.tier == "A" and c.op != "pointing":
        assert c.n_t > 2 ** 29 and 8 * c.n_t > 2 ** 32 and (c.n_det - 1) * c.n_t < 2 ** 31 < c.n_det * c.n_t
    if c.shape == "G" and c.tier == "B":                              # a lane's r * n_t + t passes 2^31 inside the second group, 2^32 inside the third
        g = c.k * c.rows * c.n_t
        assert g < 2 ** 31 < 2 * g < 2 ** 32 < 3 * g
    if c.shape == "L" and c.tier == "B":
        assert c.n_t - 1 > 2 ** 31                                    # t itself
        if c.op == "polyfilter":
            assert LT.LEAD + (c.k - 1) * LT.T_B + LT.POLY_L_OFF[-1] > 2 ** 31 and c.n_seg == 4 * c.k
        if c.op == "toeplitz":
            assert sum(s > 2 ** 31 for s in c.seg) >= 10 and len(c.seg) - 1 <= 256
        if c.op == "binfilter":
            assert (c.k - 1) * LT.T_B > 2 ** 31                       # values of order: every bin's last copies
            assert sum(c.k * int(s) > 2 ** 31 for s in c.start_b) >= 10 and sum(0 < c.k * int(s) < 2 ** 31 for s in c.start_b) >= 100


def _periods(c, name, a):
    """The tiling periods of one block array, as rows: the whole block in flat order for a wide shape; for a long one a period per
    detector row, or per (group, mode) for the amplitudes; pointing's boresight is one period either way."""
    if c.shape != "L" or name == "qb":
        return a.reshape(1, -1)
    return a.reshape(-1, LT.T_B) if name == "amps" else a.reshape(c.rows, -1)


@pytest.mark.parametrize("builder,args", CASES, ids=IDS)
def test_period(builder, args):
    """P is odd, and every Float64 array of the block -- the inputs d / x, the weights, the couplings, the kernel, the boresight, and
    the expected outputs -- rolled by 2^29, 2^31 and 2^32 mod its period, differs from itself in at least 99 % of the elements: a load
    or a store whose offset lost its high bits lands on other bits.  Three kinds of array cannot meet that over all elements and
    are held to 99 % of the elements that are not +0.0 both before and after the roll, by their definition, not by a measurement:
    random weights (one in ten is an exact zero, a cut: one pair in a hundred is two zeros), and the fit's outputs (coefficients,
    amplitudes, means: +0.0 for an empty or unfitted item; the long mode-filter case's empty group is half of them).  Not held:
    the exact-input cases' weights and integer couplings, six values each by construction, of which a roll leaves at least a sixth
    in place (their d and every output are held); the arguments a shape passes untiled (a long shape's couplings, kernel and
    detector quaternions, a wide shape's boresight); the counts
    n_used, small integers; pointing's expected outputs, which the device makes (test_gpu_large_tods.py asks the same of them
    there); and a period that divides the threshold, which only an array far shorter than the threshold has (a long polyfilter row's
    4 x (order + 1) coefficients: asserted)."""
    c = builder(*args)
    assert c.P % 2 == 1 and c.P == (c.rows * LT.T_B if c.shape in "WG" else LT.T_B)
    exact = getattr(c, "exact", False)
    untiled = ("modes", "kern", "qd", "gamma") if c.shape == "L" else ("qb",)       # passed as they are: no period, a few elements
    arrays = [(k, v, k != "w") for k, v in c.blk.items() if v is not None and k not in untiled and not (k in ("w", "modes") and exact)]
    arrays += [(k, v, k == "out") for k, v in c.exp.items() if v.dtype == np.float64]
    assert {"d", "w", "modes", "kern", "qb", "qd", "gamma"} >= {k for k, _v, _s in arrays if k not in c.exp}
    for th in LT.THRESHOLDS:
        for name, a, strict in arrays:
            for r in _periods(c, name, a):
                s = th % r.size
                if s == 0:
                    assert name == "coeffs" and c.shape == "L" and c.big.get("coeffs", 0) < 2 ** 29
                    continue
                frac, frac_nz = LT.roll_differs(r, s)
                assert (frac if strict else frac_nz) >= 0.99, (name, th, frac, frac_nz)


def test_exact_binfilter_has_the_blocks_bits_for_any_number_of_copies():
    """The long bin-filter case: the yardstick on 2 and 4 copies of the block, every bin gathering from all copies, has the block's
    bits in the sequential order and in the device's orders of 8, 64 and 256 lanes."""
    for tier in "AB":
        c = LT.binfilter("L", tier)
        assert c.exact and set(np.unique(c.blk["d"])) <= set(np.arange(-1024, 1025.0))
        for m in (2, 4):
            order, start = LT.binfilter_long_plan(c.order_b, c.start_b, m, tail=5)
            n = m * LT.T_B + 5
            assert np.array_equal(np.sort(order), np.arange(n))
            key = np.full(n, LT.N_BIN)
            for b in range(LT.N_BIN):
                key[order[start[b]:start[b + 1]]] = b
            assert np.array_equal(order, np.argsort(key, kind="stable"))                    # the stable sort bin_plan would make
            d, w = LT.tile_host(c.blk["d"], m, n=n), LT.tile_host(c.blk["w"], m, n=n)
            for lanes in (None, 8, 64, 256):
                fit = BF.filter(d, order, start, wfit=w, lanes=lanes)
                assert bits_equal(fit.out[:, :m * LT.T_B], LT.tile_host(c.exp["out"], m)), (tier, m, lanes)
                assert bits_equal(fit.out[:, m * LT.T_B:], d[:, m * LT.T_B:])
                assert bits_equal(fit.means, c.exp["means"]) and np.array_equal(fit.n_used, c.exp["n_used"])
        assert 0 < c.exp["n_used"].mean() <= 1 and np.isnan(c.blk["w"]).any() and (c.blk["w"] < 0).any()


@pytest.mark.parametrize("K", [1, 2, 3])
def test_exact_modefilter_has_the_blocks_bits_for_a_power_of_two_copies(K):
    """The giant-group case, both tiers' blocks: three groups of 2 and of 4 copies of the block have the block's bits, sequentially and
    in the device's orders of 4 and 16 row phases.  (Three copies do not for K >= 2: the LDL^T's quotients round differently.)"""
    for tier in "AB":
        c = LT.modefilter("G", tier, K)
        assert c.C == 16 and c.k & (c.k - 1) == 0 and c.n_grp * ((c.n_t + 63) // 64) < 512
        for m in (2, 4):
            d, w, F = (np.tile(c.blk[n], (3 * m, 1)) for n in ("d", "w", "modes"))
            grp = [0, m * c.rows, 2 * m * c.rows, 3 * m * c.rows]
            for phases in (None, 4, 16):
                fit = MF.filter(d, F, grp, wfit=w, rcond_min=LT.RCOND_MIN, phases=phases)
                assert bits_equal(fit.out, np.tile(c.exp["out"], (3 * m, 1))), (tier, m, phases)
                assert bits_equal(fit.amps, np.tile(c.exp["amps"], (3, 1, 1))) and np.array_equal(fit.n_used, np.tile(c.exp["n_used"], (3, 1)))
        assert (c.exp["n_used"] == K).mean() > 0.99


@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("lam", [3, 64])
def test_toeplitz_long_expectation_is_the_yardstick(tier, lam):
    """The circular result tiled, with the windows around the offsets patched in, is toeplitz_ref.apply of a row of five copies of
    the block on three long segments, bit for bit (with the cuts at tier A, without weights at tier B)."""
    c = LT.toeplitz("L", tier, lam)
    x, w, kern = c.blk["d"], c.blk["w"], c.blk["kern"]
    n_t = LT.LEAD + 5 * LT.T_B + LT.TAIL
    seg = LT.toeplitz_long_seg(n_t, 3)
    assert min(b - a for a, b in zip(seg, seg[1:])) > 4 * lam and seg[0] >= 2 * lam and seg[-1] + 2 * lam <= n_t
    want = TR.apply(LT.tile_host(x, 0, n=n_t), kern, seg, None if w is None else LT.tile_host(w, 0, n=n_t))
    got = LT.toeplitz_long_expect(x, w, kern, seg, n_t)
    assert bits_equal(got, want)
    assert not _bits(got[:, :seg[0]]).any() and not _bits(got[:, seg[-1]:]).any() and (got != 0).mean() > 0.85
    big = c.seg
    assert min(b - a for a, b in zip(big, big[1:])) > 4 * lam and big[0] >= 2 * lam and big[-1] + 2 * lam <= c.n_t
    assert all(s % TR.TILE and s % LT.T_B for s in big)


@pytest.mark.parametrize("builder,args", CASES, ids=IDS)
def test_plans_and_paths(builder, args):
    """Every plan fits 96 GiB; the host's rule selects the kernel path the case claims; the grid fits one launch."""
    c = builder(*args)
    assert c.plan_bytes <= LT.CAP_BYTES
    assert c.in_place == (c.tier == "B") if c.op not in ("toeplitz", "pointing") else True
    if c.op == "polyfilter":
        assert c.G == PF.group(c.n_t, c.n_seg, c.order) and (c.G == 256 if c.shape == "L" else 1 < c.G <= 64)
        assert (c.n_t // c.n_seg >= 1024) == (c.shape == "L")
        blocks = -(-c.n_det * (c.n_seg + 2) // (256 // c.G))
    elif c.op == "binfilter":
        assert c.G == BF.group(c.n_t, c.n_bin) and (c.G == 256 if c.shape == "L" else c.G == 64)
        blocks = -(-c.n_det * (c.n_bin + 2) // (256 // c.G))
    elif c.op == "modefilter":
        assert c.C == MF.tile(c.n_t, c.n_grp) == (16 if c.shape == "G" else 64)
        blocks = (c.n_grp + 2) * -(-c.n_t // c.C)
    elif c.op == "toeplitz":
        assert LT.toeplitz_instance(c.lam) == {3: (128, False), 64: (128, True), 1025: (4096, True)}[c.lam]
        blocks = c.n_det * -(-c.n_t // TR.TILE)
    else:
        blocks = -(-c.n_t // 256) * -(-c.n_det // 8)
    assert blocks <= 0x7fffffff
    if c.shape == "W":
        assert 10 ** 6 <= blocks <= 4 * 10 ** 7


@pytest.mark.parametrize("builder,args", LT.chunk_cases(), ids=[LT.case_id(b, a) for b, a in LT.chunk_cases()])
def test_chunk_cases_pass_one_launch(builder, args):
    """Shape C: the grid is more than one chunk of 2^24 - 8 blocks -- more than the 2^24 - 1 blocks of 256 lanes a launch can carry --
    on the kernel path the case names, the period is odd and the plan small."""
    c = builder(*args)
    assert c.shape == "W" and c.P % 2 == 1 and c.P == c.rows * c.n_t and c.plan_bytes <= 32 * LT.GIB
    if c.op == "polyfilter":
        assert c.G == PF.group(c.n_t, c.n_seg, c.order) == 64
        blocks = -(-c.n_det * (c.n_seg + 2) // (256 // c.G))
    elif c.op == "toeplitz":
        blocks = c.n_det * -(-c.n_t // TR.TILE)
    else:
        blocks = -(-c.n_t // 256) * -(-c.n_det // 8)
    assert 2 ** 24 <= LT.CHUNK_BLOCKS + 8 < blocks < LT.CHUNK_BLOCKS + 64 and LT.CHUNK_BLOCKS * 256 < 2 ** 32


def test_entries_that_do_not_chunk_refuse_a_grid_one_launch_cannot_carry(pj):
    """posmap_tan and spline_prefilter size a grid of 256-lane blocks from the map: 2^24 - 1 blocks are the most a launch carries, and
    from 2^24 on the entry refuses ("map too large for one launch") instead of running part of the grid.  Through the raw library
    on pointers that are never read: the refusal comes before the first HIP call, and one block fewer gets as far as the launch.
    Skips where a device is visible, as tests/test_abi_pointing_args.py does: an accepted call would launch on these pointers."""
    import ctypes as C
    lib = pj.load_library()
    if lib.pxl_device_count() > 0:
        pytest.skip("a GPU is visible: these calls pass pointers no kernel may touch")
    wcs = pj._lib.CarWCSStruct((C.c_double * 2)(-1 / 120.0, 1 / 120.0), (C.c_double * 2)(1.0, 1.0), (C.c_double * 2)(0.0, 0.0), np.pi / 180)

    def text():
        buf = C.create_string_buffer(512)
        lib.pxl_last_error(buf, 512)
        return buf.value.decode("utf-8", "replace")

    for ny, want in ((8 * 4095, "launch of k_posmap_tan"), (8 * 4096, "posmap_tan: map too large for one launch")):       # 4096 x ny / 8 blocks
        rc = lib.pxl_posmap_tan_f64(C.byref(wcs), (C.c_int64 * 2)(512 * 4096, ny), 0, ny, 1 << 20, 1 << 21, None)
        assert rc == (-5 if want.startswith("launch") else -22) and text().startswith(want), (ny, rc, text())
    rc = lib.pxl_spline_prefilter_car_f64(C.byref(wcs), (C.c_int64 * 3)(256 * 4096, 16 * 4096, 1), 1 << 20, (1 << 20) + (1 << 42), None)
    assert rc == -22 and text() == "spline_prefilter: map too large for one launch"
