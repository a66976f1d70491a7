"""The banded-Toeplitz noise weight on the device: pxl_tod_toeplitz_f64 and pj.toeplitz_tod against the numpy
yardstick tests/toeplitz_ref.py.

The definition fixes the order of every output's sum -- c_0 z_t first, then the taps k = 1 .. lambda one by one -- and nothing in it
depends on a tiling, so the device must give the Float64 yardstick BIT FOR BIT: there is no tolerance here.  Against the same
definition in long double every sample must also lie within toeplitz_ref.bound, (lambda + 3) 2^-52 Sabs.

Every raw call goes through an `out` with sentinels on both sides, which must stay intact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from gpu_support import dev, intact, padded, same_bits, steps, to_dev

import fit_ref
import toeplitz_ref as TR
from conftest import bits_equal

pytestmark = pytest.mark.gpu

TILE = TR.TILE
LAMBDAS = (0, 1, 3, 64, 4096)
NT_MAX = 10500


def run(pj, dev, x, kern, seg, w=None):
    """One call of the raw entry on a sentinel-padded out.  seg and kern are uploaded as they are (no host check)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    nd, nt = x.shape
    kern = np.ascontiguousarray(np.broadcast_to(kern, (nd, np.shape(kern)[-1])), dtype=np.float64)
    xd, kd = torch.from_numpy(x).to(dev), torch.from_numpy(kern).to(dev)
    sd = torch.tensor([int(v) for v in seg], dtype=torch.int64).to(dev)
    wd = None if w is None else to_dev(w, dev)
    obuf, out = padded(x.size, torch.float64, dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = pj.load_library().pxl_tod_toeplitz_f64(nd, nt, len(seg) - 1, p(sd), kern.shape[1] - 1, p(kd), p(xd), p(wd), p(out), None)
    assert rc == 0, pj._lib.last_error()
    torch.cuda.synchronize()
    assert intact(obuf, x.size), "a sentinel was overwritten"
    return out.cpu().numpy().reshape(x.shape)


def layouts(lam):
    """(name, D, T, seg_start) for one lambda.  The lengths 1, 2, lambda, lambda + 1, 2 lambda, 2 lambda + 1, C - 1, C, C + 1 and
    2 C + 1 for the kernel's tile C = 1280 and an empty segment, packed in that order into layouts of at most NT_MAX samples with a
    gap of 3 samples before the first segment and of 6 after the last; then seams exactly on a tile edge and one sample either
    side of one.  Every T is odd or prime-ish: a multiple of nothing the kernel uses."""
    nd = 3 if lam < 4096 else 2
    lengths = [1, 2, lam, lam + 1, 0, 2 * lam, 2 * lam + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
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
        lens, seams = set(), set()
        for _name, _nd, nt, seg in layouts(lam):
            assert nt <= NT_MAX and seg[0] > 0 and seg[-1] < nt
            spans = fit_ref.clamp(seg, nt)
            lens |= {hi - lo for lo, hi in spans}
            seams |= {lo % TILE for lo, _hi in spans} | {hi % TILE for _lo, hi in spans}
        assert {0, 1, 2, lam, lam + 1, 2 * lam, 2 * lam + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1} <= lens
        assert {0, 1, TILE - 1} <= seams
        assert lam < 3 or min(l for l in lens if l) < lam                           # a segment both halos leave


def make_data(nd, nt, seg, lam, seed):
    """x of rms 1 on a drift; a kernel of mixed signs that decays; weights with 10 % zeros, some negative and NaN, one whole segment
    cut (the longest); and a NaN, a +Inf and a -Inf in x under cuts of every detector."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(nd, nt)) + 10.0 * np.sin(np.arange(nt) / 300.0 + rng.uniform(0, 6, (nd, 1)))
    kern = rng.normal(size=(nd, lam + 1)) / (1.0 + np.arange(lam + 1)) ** 0.5
    w = rng.uniform(0.5, 2.0, (nd, nt)) * (rng.uniform(0, 1, (nd, nt)) >= 0.1)
    w[rng.uniform(0, 1, (nd, nt)) < 0.02] = -1.0
    w[rng.uniform(0, 1, (nd, nt)) < 0.02] = np.nan
    spans = fit_ref.clamp(seg, nt)
    lo, hi = max(spans, key=lambda s: s[1] - s[0])
    w[nd - 1, lo:hi] = 0.0
    inside = TR.live_mask((nd, nt), seg, None)
    with np.errstate(invalid="ignore"):
        cut = inside & ~(w > 0)
    for det in range(nd):
        at = np.flatnonzero(cut[det])
        x[det, at[:3]] = [np.nan, np.inf, -np.inf][:len(at[:3])]
    return x, kern, w


@functools.lru_cache(maxsize=None)
def refs(lam, name):
    """The inputs of one layout and the yardstick on them, computed once: (x, kern, w, seg, Float64 with w, Float64 without, long
    double with w, the bound with w)."""
    _n, nd, nt, seg = next(lay for lay in layouts(lam) if lay[0] == name)
    x, kern, w = make_data(nd, nt, seg, lam, 1000 + lam + len(name))
    clean = np.where(np.isfinite(x), x, 0.0)                                       # without wlive every sample is live: finite inputs
    return (x, kern, w, seg, TR.apply(x, kern, seg, w), clean, TR.apply(clean, kern, seg, None),
            TR.apply(x, kern, seg, w, dtype=np.longdouble), TR.bound(x, kern, seg, w))


@pytest.mark.parametrize("lam,layout", ALL, ids=IDS)
def test_layouts_give_the_yardsticks_bits(pj, dev, lam, layout):
    x, kern, w, seg, want, clean, want_all, ld, bound = refs(lam, layout[0])
    got = run(pj, dev, x, kern, seg, w)
    live = TR.live_mask(x.shape, seg, w)
    assert np.isfinite(got).all(), "a NaN or Inf under a cut reached an output"
    assert bits_equal(got[~live], np.zeros(int((~live).sum()))), "a cut or out-of-segment sample is not +0.0"
    same_bits(got, want, "lambda %d %s" % (lam, layout[0]))
    err = np.abs(got - ld).astype(np.float64)
    print("lambda %d %s: worst |dev - long double| / bound = %.3g" % (lam, layout[0], (err[live] / bound[live]).max()))
    assert (err <= bound).all()
    assert bits_equal(run(pj, dev, x, kern, seg, w), got)                          # a second call: the same bits
    # wlive null: every sample of a segment is live
    got_all = run(pj, dev, clean, kern, seg, None)
    same_bits(got_all, want_all, "lambda %d %s, wlive null" % (lam, layout[0]))
    inside = TR.live_mask(x.shape, seg, None)
    assert bits_equal(got_all[~inside], np.zeros(int((~inside).sum())))
    assert bits_equal(run(pj, dev, clean, kern, seg, np.ones_like(clean)), got_all)


@pytest.mark.parametrize("lam", [16, 17, 128, 129, 1024, 1025])
def test_every_instantiation_on_both_sides_of_its_limit(pj, dev, lam):
    """The kernel is instantiated for lambda <= 128, <= 1024 and <= 4096 (the size of its LDS), and from lambda = 17 on a lane
    carries consecutive outputs behind sliding windows: the last lambda of one form and the first of the next, on three segments
    that cut tiles."""
    nd, nt, seg = 2, 2 * TILE + 611, [7, 700, 700 + lam, 2 * TILE + 600]
    x, kern, w = make_data(nd, nt, seg, lam, 7 + lam)
    got = run(pj, dev, x, kern, seg, w)
    same_bits(got, TR.apply(x, kern, seg, w), "lambda %d" % lam)
    assert np.isfinite(got).all()


def test_more_segments_than_one_round_of_the_search(pj, dev):
    """A block looks through the segments 256 at a time: 430 segments of 7 samples and one of 1500, at lambda = 3."""
    nd, lam = 2, 3
    seg = steps([7] * 300 + [1500] + [7] * 130, start=2)
    nt = seg[-1] + 3
    x, kern, w = make_data(nd, nt, seg, lam, 77)
    same_bits(run(pj, dev, x, kern, seg, w), TR.apply(x, kern, seg, w), "431 segments")


def test_seg_start_in_any_order_and_outside_the_timestream(pj, dev):
    """Built by hand for the raw entry.  Segments that do not overlap are found in any order, and offsets below 0 and past n_t are
    clamped: the yardstick's segments and its bits.  Offsets near +-2^62 in any order make overlapping segments, whose values the
    header leaves open: the call must stay inside its buffers (run's sentinels); nothing else is asked of it."""
    nd, nt, lam = 2, 2 * TILE + 300, 64
    for seg in ([1500, 2100, 0, 1500], [-5, 400, 5000, 2 ** 62], [2000, 2348, 900, 1100, 1100, 2000, 10, 900]):
        spans = [s for s in fit_ref.clamp(seg, nt) if s[1] > s[0]]
        assert all(a[1] <= b[0] or b[1] <= a[0] for i, a in enumerate(spans) for b in spans[i + 1:])
        x, kern, w = make_data(nd, nt, seg, lam, 5 + len(seg))
        same_bits(run(pj, dev, x, kern, seg, w), TR.apply(x, kern, seg, w), str(seg))
    x, kern, w = make_data(nd, nt, [0, nt], lam, 9)
    wild = run(pj, dev, np.where(np.isfinite(x), x, 0.0), kern, [90, -2 ** 62, 2 ** 62, 17, 150, -1, 60, -2 ** 63, 2 ** 63 - 1, 0], w)
    assert np.isfinite(wild).all()


@pytest.mark.parametrize("lam", [3, 64, 4096])
def test_a_live_nan_reaches_lambda_samples_in_its_segment_and_no_others(pj, dev, lam):
    """A NaN (or an Inf: Inf * c_k - Inf * c_k' is NaN or Inf) at a live sample makes exactly the live samples within lambda of it
    in its own segment non-finite, and changes no other sample's bits."""
    nd = 2
    seg = [3, 2000, 2000 + min(lam, 900) + 40, 4100]
    nt = 4111
    rng = np.random.default_rng(lam)
    x = rng.normal(size=(nd, nt))
    kern = rng.uniform(0.5, 1.0, (nd, lam + 1))                                    # no zero tap: every neighbour is reached
    w = (rng.uniform(0, 1, (nd, nt)) >= 0.1).astype(np.float64)
    base = run(pj, dev, x, kern, seg, w)
    for det, t, bad in ((0, 1990, np.nan), (1, 2010, np.inf), (0, 3, -np.inf)):
        w2 = w.copy()
        w2[det, t] = 1.0
        ref = run(pj, dev, x, kern, seg, w2) if w[det, t] == 0 else base
        x2 = x.copy()
        x2[det, t] = bad
        got = run(pj, dev, x2, kern, seg, w2)
        lo, hi = next(s for s in fit_ref.clamp(seg, nt) if s[0] <= t < s[1])
        reach = np.zeros((nd, nt), dtype=bool)
        reach[det, max(lo, t - lam):min(hi, t + lam + 1)] = True
        reach &= TR.live_mask(x.shape, seg, w2)
        assert reach[det, t] and not np.isfinite(got[reach]).any()
        assert bits_equal(got[~reach], ref[~reach])
        same_bits(got, TR.apply(x2, kern, seg, w2), "live %r" % bad)


def test_the_python_wrapper_is_the_same_call(pj, dev):
    """One layout through pj.toeplitz_tod: a (lambda + 1,) kernel for every detector, (D, T) and (D,) weights, seg_start a list, a
    CPU tensor and None, out given and not; out on tod is refused."""
    lam, (_name, nd, nt, seg) = 64, layouts(64)[0]
    x, kern, w = make_data(nd, nt, seg, lam, 123)
    x = np.where(np.isfinite(x), x, 0.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    want = TR.apply(x, kern[0], seg, w)
    got = pj.toeplitz_tod(t(x), t(kern[0]), seg, w=t(w))
    same_bits(got.cpu().numpy(), want, "wrapper")
    assert bits_equal(got.cpu().numpy(), run(pj, dev, x, kern[0], seg, w))
    same_bits(pj.toeplitz_tod(t(x), t(kern), torch.tensor(seg), w=t(w)).cpu().numpy(), TR.apply(x, kern, seg, w), "per-detector kernel")
    wdet = np.array([1.0, 0.0, 2.5])[:nd]
    buf = torch.full((nd, nt), 7.0, dtype=torch.float64, device=dev)
    assert pj.toeplitz_tod(t(x), t(kern[0]), None, w=t(wdet), out=buf) is buf
    same_bits(buf.cpu().numpy(), TR.apply(x, kern[0], [0, nt], np.repeat(wdet[:, None], nt, axis=1)), "one segment, (D,) weights")
    arena = torch.zeros((nd * nt + 1,), dtype=torch.float64, device=dev)
    for out in (arena[1:].view(nd, nt), arena[:nd * nt].view(nd, nt)):
        with pytest.raises(ValueError, match="out may not"):
            pj.toeplitz_tod(arena[:nd * nt].view(nd, nt), t(kern[0]), seg, out=out)
