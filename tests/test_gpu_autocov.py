"""The gappy autocovariance on the device: pxl_tod_autocov_f64 and pj.autocov_tod against the numpy yardstick
tests/autocov_ref.py.

The header fixes the order of every sum from lambda, n_t and seg_start alone, and the yardstick restates it, so the device must give
the Float64 yardstick BIT FOR BIT and the pair counts exactly: there is no tolerance here.  Against the same sums in long double every
value must also lie within autocov_ref.bound, (pairs_k + 2) 2^-52 sum |z_t z_(t+k)|.

Every raw call writes `sums` and `pairs` between sentinels, which must stay intact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from gpu_support import dev, intact, padded, same_bits, steps, to_dev
from test_gpu_toeplitz import make_data

import autocov_ref as AR
import fit_ref
import toeplitz_ref as TR
from conftest import bits_equal

pytestmark = pytest.mark.gpu

TILE = AR.TILE
LAMBDAS = (0, 1, 3, 64, 4096)
NT_MAX = 10500


def run(pj, dev, x, lam, seg, w=None, with_pairs=True):
    """One call of the raw entry on sentinel-padded sums and pairs.  seg is uploaded as it is (no host check).  Returns (sums,
    pairs), pairs None without them."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    nd, nt = x.shape
    xd = torch.from_numpy(x).to(dev)
    sd = torch.tensor([int(v) for v in seg], dtype=torch.int64).to(dev)
    wd = None if w is None else to_dev(w, dev)
    n = nd * (lam + 1)
    sbuf, sums = padded(n, torch.float64, dev)
    pbuf, pairs = padded(n, torch.int64, dev)
    p = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
    rc = pj.load_library().pxl_tod_autocov_f64(nd, nt, len(seg) - 1, p(sd), lam, p(xd), p(wd), p(sums), p(pairs) if with_pairs else None, None)
    assert rc == 0, pj._lib.last_error()
    torch.cuda.synchronize()
    assert intact(sbuf, n) and intact(pbuf, n), "a sentinel was overwritten"
    if not with_pairs:
        assert bool((pairs == pbuf[0]).all()), "pairs was written though null was passed"
    return sums.cpu().numpy().reshape(nd, lam + 1), pairs.cpu().numpy().reshape(nd, lam + 1) if with_pairs else None


def layouts(lam):
    """(name, D, T, seg_start) for one lambda.  The lengths 1, 2, lambda, lambda + 1, 2 lambda + 1, C - 1, C, C + 1 and 2 C + 1 for
    the kernel's time tile C = 1280 and an empty segment, packed in that order into layouts of at most NT_MAX samples with a gap of
    3 samples before the first segment and of 6 after the last.  The kernel's tiles start at a segment's first sample, so the
    lengths C - 1, C and C + 1 (and 2 C + 1) ARE the seams on a tile edge and one sample either side; `seams` adds segment ends on
    the multiples of C of the time axis itself and next to them.  Every T is odd or prime-ish: a multiple of nothing the kernel
    uses."""
    nd = 3 if lam < 4096 else 2
    lengths = [1, 2, lam, lam + 1, 0, 2 * lam + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
    packs, cur = [], []
    for L in lengths:
        if cur and sum(cur) + L + 9 > NT_MAX:
            packs.append(cur)
            cur = []
        cur.append(L)
    packs.append(cur)
    out = [("lengths%d" % i, nd, sum(p) + 9, steps(p, start=3)) for i, p in enumerate(packs)]
    out.append(("seams", nd, 3 * TILE + 539, [5, TILE - 1, 2 * TILE, 3 * TILE + 1, 3 * TILE + 500]))
    return out


ALL = [(lam, lay) for lam in LAMBDAS for lay in layouts(lam)]
IDS = ["l%d-%s" % (lam, lay[0]) for lam, lay in ALL]


def test_the_layouts_hold_what_they_promise():
    for lam in LAMBDAS:
        lens, ends = set(), set()
        for _name, _nd, nt, seg in layouts(lam):
            assert nt <= NT_MAX and seg[0] > 0 and seg[-1] < nt
            spans = fit_ref.clamp(seg, nt)
            lens |= {hi - lo for lo, hi in spans}
            ends |= {(hi - lo) % TILE for lo, hi in spans if hi - lo >= TILE - 1}     # where a segment ends in the tiles that start at lo
            ends |= {("axis", hi % TILE) for _lo, hi in spans}
        assert {0, 1, 2, lam, lam + 1, 2 * lam + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1} <= lens
        assert {TILE - 1, 0, 1} <= ends and {("axis", TILE - 1), ("axis", 0), ("axis", 1)} <= ends
        assert lam < 3 or min(l for l in lens if l) < lam                           # a segment shorter than the lags


@functools.lru_cache(maxsize=None)
def refs(lam, name):
    """The inputs of one layout and the yardstick on them, computed once: (x, w, seg, Float64 sums with w, pairs with w, the finite
    x, Float64 sums and pairs without w, long double sums with w, the bound with w)."""
    _n, nd, nt, seg = next(lay for lay in layouts(lam) if lay[0] == name)
    x, _kern, w = make_data(nd, nt, seg, 0, 2000 + lam + len(name))
    clean = np.where(np.isfinite(x), x, 0.0)                                       # without wlive every sample is live: finite inputs
    return (x, w, seg, AR.sums(x, lam, seg, w), AR.pairs(x.shape, lam, seg, w), clean, AR.sums(clean, lam, seg, None),
            AR.pairs(x.shape, lam, seg, None), AR.sums(x, lam, seg, w, dtype=np.longdouble), AR.bound(x, lam, seg, w))


@pytest.mark.parametrize("lam,layout", ALL, ids=IDS)
def test_layouts_give_the_yardsticks_bits(pj, dev, lam, layout):
    x, w, seg, want, npairs, clean, want_all, npairs_all, ld, bound = refs(lam, layout[0])
    got, gp = run(pj, dev, x, lam, seg, w)
    assert np.isfinite(got).all(), "a NaN or Inf under a cut reached a sum"
    assert np.array_equal(gp, npairs), "pairs"
    same_bits(got, want, "lambda %d %s" % (lam, layout[0]))
    assert bits_equal(got[npairs == 0], np.zeros(int((npairs == 0).sum()))), "a lag with no pair is not +0.0"
    err = np.abs(got - ld).astype(np.float64)
    some = npairs > 0
    print("lambda %d %s: worst |dev - long double| / bound = %.3g" % (lam, layout[0], (err[some] / bound[some]).max()))
    assert (err <= bound).all()
    again, gp2 = run(pj, dev, x, lam, seg, w)                                       # a second call: the same bits
    assert bits_equal(again, got) and np.array_equal(gp2, gp)
    alone, none = run(pj, dev, x, lam, seg, w, with_pairs=False)                    # pairs null: sums unchanged
    assert none is None and bits_equal(alone, got)
    # wlive null: every sample of a segment is live
    got_all, gp_all = run(pj, dev, clean, lam, seg, None)
    same_bits(got_all, want_all, "lambda %d %s, wlive null" % (lam, layout[0]))
    assert np.array_equal(gp_all, npairs_all)
    ones, gp_ones = run(pj, dev, clean, lam, seg, np.ones_like(clean))
    assert bits_equal(ones, got_all) and np.array_equal(gp_ones, gp_all)


@pytest.mark.parametrize("lam", AR.FORM_EDGES)
def test_every_form_on_both_sides_of_its_limit(pj, dev, lam):
    """The lanes of a group double at lambda = 5, 10, 20 .. 640 (P partials and their tree halve), and the lags fill a second, third
    and fourth block from 1280, 2560 and 3840 on: the last lambda of one form and the first of the next, on three segments that
    cut tiles, the last one longer than every lag."""
    nd, nt = 2, 3 * TILE + 611 + lam
    seg = [7, 700, 700 + lam % 1000 + 3, nt - 11]
    x, _kern, w = make_data(nd, nt, seg, 0, 7 + lam)
    got, gp = run(pj, dev, x, lam, seg, w)
    want = AR.pairs(x.shape, lam, seg, w)
    assert np.array_equal(gp, want) and (want[0] > 0).all()
    same_bits(got, AR.sums(x, lam, seg, w), "lambda %d" % lam)
    assert np.isfinite(got).all()


def test_many_short_segments_and_a_long_one(pj, dev):
    """A block walks every segment in the order of s (there are no rounds of a search): 430 segments of 7 samples and one of 1500, at
    lambda = 3 and 64."""
    seg = steps([7] * 300 + [1500] + [7] * 130, start=2)
    nd, nt = 2, seg[-1] + 3
    for lam in (3, 64):
        x, _kern, w = make_data(nd, nt, seg, 0, 77 + lam)
        got, gp = run(pj, dev, x, lam, seg, w)
        assert np.array_equal(gp, AR.pairs(x.shape, lam, seg, w))
        same_bits(got, AR.sums(x, lam, seg, w), "431 segments, lambda %d" % lam)


def test_seg_start_in_any_order_and_outside_the_timestream(pj, dev):
    """Built by hand for the raw entry.  Offsets below 0 and past n_t are clamped, and empty (reversed) segments add nothing: the
    yardstick's segments, in seg_start's order, and its bits.  Offsets near +-2^62 in any order make overlapping segments, whose
    values the header leaves open: the call must stay inside its buffers (run's sentinels); nothing else is asked of it."""
    nd, nt, lam = 2, 2 * TILE + 300, 64
    for seg in ([1500, 2100, 0, 1500], [-5, 400, 5000, 2 ** 62], [2000, 2348, 900, 1100, 1100, 2000, 10, 900]):
        spans = [s for s in fit_ref.clamp(seg, nt) if s[1] > s[0]]
        assert all(a[1] <= b[0] or b[1] <= a[0] for i, a in enumerate(spans) for b in spans[i + 1:])
        x, _kern, w = make_data(nd, nt, seg, 0, 5 + len(seg))
        got, gp = run(pj, dev, x, lam, seg, w)
        assert np.array_equal(gp, AR.pairs(x.shape, lam, seg, w))
        same_bits(got, AR.sums(x, lam, seg, w), str(seg))
    x, _kern, w = make_data(nd, nt, [0, nt], 0, 9)
    for lam in (3, 64, 2000):
        wild, _gp = run(pj, dev, np.where(np.isfinite(x), x, 0.0), lam, [90, -2 ** 62, 2 ** 62, 17, 150, -1, 60, -2 ** 63, 2 ** 63 - 1, 0], w)
        assert np.isfinite(wild).all()


@pytest.mark.parametrize("lam", [3, 64, 1500])
def test_a_row_alone_has_the_bits_it_has_in_a_batch(pj, dev, lam):
    """Every row of a D = 3 call equals, bit for bit, the D = 1 call on that row, and the rows permuted give the permuted result."""
    nd, nt = 3, 2 * TILE + 777
    seg = [4, 1000, 1000 + TILE + 1, nt - 2]
    x, _kern, w = make_data(nd, nt, seg, 0, 31 + lam)
    got, gp = run(pj, dev, x, lam, seg, w)
    for r in range(nd):
        one, p1 = run(pj, dev, x[r:r + 1], lam, seg, w[r:r + 1])
        assert bits_equal(one[0], got[r]) and np.array_equal(p1[0], gp[r]), r
    perm = [2, 0, 1]
    moved, pm = run(pj, dev, x[perm], lam, seg, w[perm])
    assert bits_equal(moved, got[perm]) and np.array_equal(pm, gp[perm])


@pytest.mark.parametrize("lam", [3, 64, 4096])
def test_a_live_nan_stays_in_its_detector(pj, dev, lam):
    """A NaN or an Inf at a live sample makes lag 0 of its detector non-finite and changes no bit of the other detector."""
    nd, nt = 2, 4111
    seg = [3, 2000, 2000 + min(lam, 900) + 40, 4100]
    rng = np.random.default_rng(lam)
    x = rng.normal(size=(nd, nt))
    w = (rng.uniform(0, 1, (nd, nt)) >= 0.1).astype(np.float64)
    for det, t, bad in ((0, 1990, np.nan), (1, 2010, np.inf), (0, 3, -np.inf)):
        w2 = w.copy()
        w2[det, t] = 1.0
        base, bp = run(pj, dev, x, lam, seg, w2)
        x2 = x.copy()
        x2[det, t] = bad
        got, gp = run(pj, dev, x2, lam, seg, w2)
        assert not np.isfinite(got[det, 0])
        assert bits_equal(got[1 - det], base[1 - det]) and np.array_equal(gp, bp)


def test_no_samples_still_zero_the_outputs(pj, dev):
    """n_t = 0 with detectors and lags: sums +0.0 and pairs 0, every element, and nothing beyond."""
    for with_pairs in (True, False):
        got, gp = run(pj, dev, np.zeros((3, 0)), 5, [0, 0], None, with_pairs)
        assert bits_equal(got, np.zeros((3, 6))) and (gp is None or not gp.any())


def test_the_python_wrapper_is_the_same_call(pj, dev):
    """One layout through pj.autocov_tod: (D, T) and (D,) weights, seg_start a list, a CPU tensor and None, with and without pairs."""
    lam, (_name, nd, nt, seg) = 64, layouts(64)[0]
    x, _kern, w = make_data(nd, nt, seg, 0, 123)
    x = np.where(np.isfinite(x), x, 0.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    want, npairs = AR.sums(x, lam, seg, w), AR.pairs(x.shape, lam, seg, w)
    sums, pairs = pj.autocov_tod(t(x), lam, seg, w=t(w))
    assert sums.dtype == torch.float64 and pairs.dtype == torch.int64 and tuple(sums.shape) == tuple(pairs.shape) == (nd, lam + 1)
    same_bits(sums.cpu().numpy(), want, "wrapper")
    assert np.array_equal(pairs.cpu().numpy(), npairs)
    raw, _rp = run(pj, dev, x, lam, seg, w)
    assert bits_equal(sums.cpu().numpy(), raw)
    alone = pj.autocov_tod(t(x), lam, torch.tensor(seg), w=t(w), return_pairs=False)
    assert isinstance(alone, torch.Tensor) and bits_equal(alone.cpu().numpy(), want)
    wdet = np.array([1.0, 0.0, 2.5])[:nd]
    wfull = np.repeat(wdet[:, None], nt, axis=1)
    sums, pairs = pj.autocov_tod(t(x), lam, None, w=t(wdet))
    same_bits(sums.cpu().numpy(), AR.sums(x, lam, [0, nt], wfull), "one segment, (D,) weights")
    assert np.array_equal(pairs.cpu().numpy(), AR.pairs(x.shape, lam, [0, nt], wfull)) and not pairs[1].any()
    sums, pairs = pj.autocov_tod(t(x), 0)
    same_bits(sums.cpu().numpy(), AR.sums(x, 0, [0, nt]), "lambda 0, no weights")
    assert (pairs.cpu().numpy() == nt).all()
    with pytest.raises(ValueError, match=r"w is \(D, T\) or \(D,\)"):
        pj.autocov_tod(t(x), lam, seg, w=t(w[:, :-1]))
