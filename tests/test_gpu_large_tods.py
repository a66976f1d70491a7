"""The timestream kernels on (D, T) buffers whose flat element offsets det * n_t + t pass 2^29, 2^31 and 2^32:
k_polyfilter, k_modefilter, k_binfilter, k_toeplitz and k_pointing_expand, through their raw entries on device tensors
(gpu_support.call_entry), and the four filters' Python wrappers once each.

The cases, their sizes and the method -- a checked block, tiled; technique 1 of test_gpu_second_trip.py -- are stated in
tests/large_tod_case.py and shown on the CPU by tests/test_large_tod_case.py.  Sizes chosen: T_B = 10007 samples; blocks of 21 rows
(wide shapes), 71 rows (the mode filter's giant groups), 11 and 8 detectors (pointing_expand); long rows of
1531 + k 10007 + 4099 samples.  Here the device tiles the block into the big arguments (expand / copy_ and arange arithmetic;
nothing dense exists on the host), every output starts as a NaN with a payload, ONE call runs, and every element of every output is
compared on the device, as int64, with the tiling of the block's expectation, at most 2^27 elements at a time (`held`).  A NaN
is expected exactly where the yardstick has one (gpu_support.same_bits' rule: a NaN's payload is the adder's own), and an
element that still holds the sentinel's payload counts as wrong wherever it is.  Each test asserts that the elements it compared
are all the elements of the buffer.

Shape C (polyfilter, Toeplitz, pointing_expand on short rows tiled to 2^24 + 16 blocks) holds the second chunk of a grid that one
launch cannot carry: the first run of this file found that a launch of more than 2^24 - 1 blocks of 256 lanes runs only part of its
grid, through the wide tier-B bin filter and the long mode filter (NOTES.md).

pointing_expand's outputs are double2, 16 bytes an element: past 2^32 elements they would be 128 GiB, so it has tier A alone.  Its
expectation is the device's own call on the block, first held to pointing_ref under test_gpu_pointing.py's bound.

Every test allocates inside try / finally, skips with both figures when the device has less free memory than its plan plus
8 GiB, plans at most 96 GiB (asserted), and prints a line `large-tod: ...` with the result, the elements compared, the peak device
memory and the seconds."""
import time

import numpy as np
import pytest

import large_tod_case as LT
import pointing_ref as PR
from large_tod_case import T_B

torch = pytest.importorskip("torch")
from gpu_support import begin_large, call_entry, dev, same_bits, to_dev
from test_gpu_pointing import bound
pytestmark = pytest.mark.gpu

I64, F64 = torch.int64, torch.float64


class Bufs:
    """The big tensors of one test, so that `finally` can drop every reference to them."""


def _begin(dev, c, what, extra_bytes=0):
    return begin_large(dev, c.plan_bytes + extra_bytes, what, LT.CAP_BYTES)


def _report(what, t0, dev, compared):
    torch.cuda.synchronize()
    print("large-tod: %s: bits, %d elements compared, %.1f GB peak, %.1f s" % (what, compared, torch.cuda.max_memory_allocated(dev) / 1e9, time.time() - t0))


def _release(m):
    m.__dict__.clear()
    torch.cuda.empty_cache()


def sentinel(n, dev, dtype=F64):
    """n elements that hold the sentinel: a NaN with a payload for Float64, the same bits for an int64 count."""
    return torch.full((n,), LT.SENTINEL_BITS, dtype=I64, device=dev).view(dtype)


def tile_row(dst, blk, lead=0):
    """dst[t] = blk[(t - lead) mod p] for the 1-D device tensors dst (n) and blk (p): whole copies by expand / copy_."""
    p, n = blk.numel(), dst.numel()
    h = min(lead % p, n)
    if h:
        dst[:h].copy_(blk[p - lead % p:p - lead % p + h])
    m = (n - h) // p
    if m:
        dst[h:h + m * p].view(m, p).copy_(blk.unsqueeze(0).expand(m, p))
    if n - h - m * p:
        dst[h + m * p:].copy_(blk[:n - h - m * p])


def tiled(blk, rows, n, dev, lead=0):
    """The (rows, n) device tensor whose row r tiles row r of the host block (rows, p); rows = 1 tiles the whole block in flat order."""
    b = to_dev(blk, dev, dtype=blk.dtype).reshape(rows, -1)
    out = torch.empty((rows, n), dtype=b.dtype, device=dev)
    for r in range(rows):
        tile_row(out[r], b[r], lead)
    return out


def _mismatch(got, blk, lead, lo, hi, is_float):
    """got, blk: 1-D int64 device tensors.  (how many i in [lo, hi) have got[i] != blk[(i - lead) mod p] or still hold the sentinel,
    the first such i or -1).  Two NaNs compare equal where is_float."""
    p = blk.numel()
    nan = torch.isnan(blk.view(F64)) if is_float else None
    nbad, first = 0, -1

    def cmp(g, e, en, at):
        nonlocal nbad, first
        bad = g != e
        if is_float:
            bad &= ~(en & torch.isnan(g.view(F64)))
        bad |= g == LT.SENTINEL_BITS
        n = int(bad.sum())
        if n and first < 0:
            first = at + int(torch.nonzero(bad.reshape(-1))[0])
        nbad += n

    i, off = lo, (lo - lead) % p
    if off and i < hi:
        n = min(p - off, hi - i)
        cmp(got[i:i + n], blk[off:off + n], nan[off:off + n] if is_float else None, i)
        i += n
    rows = max(1, LT.SLAB // p)
    while hi - i >= p:
        m = min(rows, (hi - i) // p)
        cmp(got[i:i + m * p].view(m, p), blk[None, :], nan[None, :] if is_float else None, i)
        i += m * p
    if i < hi:
        cmp(got[i:hi], blk[:hi - i], nan[:hi - i] if is_float else None, i)
    return nbad, first


def held(what, t, spans):
    """Every element of the (rows, n) device tensor t (Float64 or int64) against tilings of host blocks.  spans: [(lo, hi, blk,
    lead)]: for every row r and i in [lo, hi), t[r, i] must have the bits of blk[r, (i - lead) mod p], blk (rows, p); a blk of
    one row serves every row.  Returns the number of elements compared; the spans must cover [0, n) exactly."""
    rows, n = t.shape
    is_float = t.dtype == F64
    bits = t.view(I64)
    compared, fail = 0, None
    at = 0
    for lo, hi, blk, lead in spans:
        assert lo == at and hi >= lo, "the spans leave a gap"
        at = hi
        b = np.ascontiguousarray(blk, dtype=np.float64 if is_float else np.int64).view(np.int64)
        b = torch.from_numpy(b.reshape(b.shape[0], -1)).to(t.device)
        for r in range(rows):
            nbad, first = _mismatch(bits[r], b[r % b.shape[0]], lead, lo, hi, is_float)
            compared += hi - lo
            if nbad and fail is None:
                p = b.shape[1]
                fail = "%s: %d elements of row %d in [%d, %d) differ; the first at flat index %d = row %d, sample %d, phase %d of the period %d" % (
                    what, nbad, r, lo, hi, r * n + first, r, first, (first - lead) % p, p)
        del b
    assert at == n, "the spans do not reach the end"
    del bits
    assert fail is None, fail
    return compared


def whole(blk, n, lead=0):
    """The one span that tiles blk over a whole row."""
    return [(0, n, blk, lead)]


def flat(t):
    return t.reshape(1, -1)


def _filter_inputs(m, c, dev):
    """m.d, m.w (None without weights) and m.out of a filter case: the block tiled, out the sentinel or, in place, d itself."""
    rows = c.n_det if c.shape == "L" else 1
    n = c.n_det * c.n_t // rows
    m.d = tiled(c.blk["d"], rows, n, dev, c.lead)
    m.w = None if c.blk["w"] is None else tiled(c.blk["w"], rows, n, dev, c.lead)
    m.out = m.d if c.in_place else sentinel(c.n_det * c.n_t, dev).view(rows, n)


def _arange_offsets(k, step, offs, last, dev, start=0):
    """start + i * step + offs[j] for i < k and every j, in that order, then `last`: offsets tiled with the block."""
    o = start + torch.arange(k, dtype=I64, device=dev)[:, None] * step + torch.tensor(offs, dtype=I64, device=dev)[None, :]
    return torch.cat([o.reshape(-1), torch.tensor([last], dtype=I64, device=dev)])


# ================================================================================================
# polyfilter
# ================================================================================================

def _polyfilter_setup(m, c, dev):
    _filter_inputs(m, c, dev)
    if c.shape == "W":
        m.seg = torch.tensor(c.seg, dtype=I64, device=dev)
    else:
        m.seg = _arange_offsets(c.k, T_B, LT.POLY_L_OFF, c.lead + c.k * T_B, dev, start=c.lead)
    assert m.seg.numel() == c.n_seg + 1
    np1 = c.order + 1
    m.coeffs = None if c.in_place else sentinel(c.n_det * c.n_seg * np1, dev)
    m.n_used = None if c.in_place else sentinel(c.n_det * c.n_seg, dev, I64)


def _polyfilter_out_spans(c):
    if c.shape == "W":
        return whole(c.exp["out"].reshape(1, -1), c.n_det * c.n_t)
    end = c.lead + c.k * T_B                                          # before the first offset and from the last on: copied
    return [(0, c.lead, c.blk["d"], c.lead), (c.lead, end, c.exp["out"], c.lead), (end, c.n_t, c.blk["d"], c.lead)]


def _polyfilter_fit_held(what, c, coeffs, n_used):
    rows = c.n_det if c.shape == "L" else 1
    n = held(what + ", coeffs", coeffs.reshape(rows, -1), whole(c.exp["coeffs"].reshape(rows, -1), coeffs.numel() // rows))
    return n + held(what + ", n_used", n_used.reshape(rows, -1), whole(c.exp["n_used"].reshape(rows, -1), n_used.numel() // rows))


POLY = [(s, t, o) for t in "AB" for s, orders in (("W", (0, 3)), ("L", (1, 7))) for o in orders] + [("C", "A", 0)]


@pytest.mark.parametrize("shape,tier,order", POLY, ids=["%s-%s-o%d" % p for p in POLY])
def test_polyfilter(pj, dev, shape, tier, order):
    """k_polyfilter<order>.  W: 17 segments a row, G = 64, 10^6 blocks and more; L: four segments per copy of the block, G = 256,
    seg_start up to n_t.  Tier A: wfit, a separate out, coeffs and n_used; tier B: in place with wfit."""
    c = LT.polyfilter(shape, tier, order)
    what = "polyfilter %s %s order %d (%d x %d, G = %d)" % (shape, tier, order, c.n_det, c.n_t, c.G)
    shape = c.shape                                                   # a chunk case reads as a wide one
    t0 = _begin(dev, c, what)
    m = Bufs()
    try:
        _polyfilter_setup(m, c, dev)
        call_entry(pj, "pxl_tod_polyfilter_f64", c.n_det, c.n_t, c.n_seg, m.seg, order, LT.RCOND_MIN, m.d, m.w, m.out, m.coeffs, m.n_used)
        n = held(what, m.out, _polyfilter_out_spans(c))
        assert n == c.n_det * c.n_t
        if not c.in_place:
            assert _polyfilter_fit_held(what, c, m.coeffs, m.n_used) == c.n_det * c.n_seg * (order + 2)
            n += c.n_det * c.n_seg * (order + 2)
        _report(what, t0, dev, n)
    finally:
        _release(m)


# ================================================================================================
# binfilter
# ================================================================================================

def _long_order(c, dev):
    """large_tod_case.binfilter_long_plan on the device, bin by bin: block positions plus i * T_B."""
    order = torch.empty((c.n_t,), dtype=I64, device=dev)
    base = (torch.arange(c.k, dtype=I64, device=dev) * T_B)[:, None]
    at = 0
    for b in range(c.n_bin + 1):
        pos = c.order_b[c.start_b[b]:c.start_b[b + 1] if b < c.n_bin else T_B]
        if len(pos):
            order[at:at + c.k * len(pos)].view(c.k, len(pos)).copy_(base + torch.from_numpy(pos).to(dev)[None, :])
            at += c.k * len(pos)
    assert at == c.k * T_B
    order[at:] = torch.arange(at, c.n_t, dtype=I64, device=dev)
    return order, torch.from_numpy(c.k * c.start_b).to(dev)


def _binfilter_setup(m, c, dev):
    _filter_inputs(m, c, dev)
    if c.shape == "W":
        m.order, m.start = torch.from_numpy(c.order_b).to(dev), torch.from_numpy(c.start_b).to(dev)
    else:
        m.order, m.start = _long_order(c, dev)
    m.means = None if c.in_place else sentinel(c.n_det * c.n_bin, dev)
    m.n_used = None if c.in_place else sentinel(c.n_det * c.n_bin, dev, I64)


def _binfilter_out_spans(c):
    if c.shape == "W":
        return whole(c.exp["out"].reshape(1, -1), c.n_det * c.n_t)
    return [(0, c.k * T_B, c.exp["out"], 0), (c.k * T_B, c.n_t, c.blk["d"], 0)]          # the tail is in no bin: copied


def _binfilter_fit_held(what, c, means, n_used):
    rows = c.n_det if c.shape == "L" else 1
    n = held(what + ", means", means.reshape(rows, -1), whole(c.exp["means"].reshape(rows, -1), means.numel() // rows))
    return n + held(what + ", n_used", n_used.reshape(rows, -1), whole(c.exp["n_used"].reshape(rows, -1), n_used.numel() // rows))


@pytest.mark.parametrize("shape,tier", [(s, t) for t in "AB" for s in "WL"], ids=lambda v: v)
def test_binfilter(pj, dev, shape, tier):
    """k_binfilter.  W: the block's plan shared by 10^5 rows, random reals, G = 64, 10^7 blocks (the unsigned XCD remap).  L: 300 bins
    that each gather from all k copies of the block (G = 256), exact inputs, order and bin_start up to n_t."""
    c = LT.binfilter(shape, tier)
    what = "binfilter %s %s (%d x %d, G = %d)" % (shape, tier, c.n_det, c.n_t, c.G)
    t0 = _begin(dev, c, what)
    m = Bufs()
    try:
        _binfilter_setup(m, c, dev)
        call_entry(pj, "pxl_tod_binfilter_f64", c.n_det, c.n_t, c.n_bin, m.start, m.order, m.d, m.w, m.out, m.means, m.n_used)
        n = held(what, m.out, _binfilter_out_spans(c))
        assert n == c.n_det * c.n_t
        if not c.in_place:
            assert _binfilter_fit_held(what, c, m.means, m.n_used) == 2 * c.n_det * c.n_bin
            n += 2 * c.n_det * c.n_bin
        _report(what, t0, dev, n)
    finally:
        _release(m)


# ================================================================================================
# modefilter
# ================================================================================================

def _modefilter_setup(m, c, dev):
    _filter_inputs(m, c, dev)
    K = c.K
    if c.shape == "W":
        m.modes = tiled(c.blk["modes"], 1, c.n_det * K, dev)
        m.grp = _arange_offsets(c.k, c.rows, c.grp_b[:-1], c.n_det, dev)
    elif c.shape == "G":
        m.modes = tiled(c.blk["modes"], 1, c.n_det * K, dev)
        m.grp = torch.tensor([0, c.k * c.rows, 2 * c.k * c.rows, 3 * c.k * c.rows], dtype=I64, device=dev)
    else:
        m.modes = to_dev(c.blk["modes"], dev)
        m.grp = torch.tensor(c.grp_b, dtype=I64, device=dev)
    assert m.grp.numel() == c.n_grp + 1
    m.amps = None if c.in_place else sentinel(c.n_grp * K * c.n_t, dev)
    m.n_used = None if c.in_place else sentinel(c.n_grp * c.n_t, dev, I64)


def _modefilter_out_spans(c):
    if c.shape == "L":
        return whole(c.exp["out"], c.n_t, c.lead)
    return whole(c.exp["out"].reshape(1, -1), c.n_det * c.n_t)


def _modefilter_fit_held(what, c, amps, n_used):
    ea, eu = c.exp["amps"], c.exp["n_used"]
    if c.shape == "G":                                                # the three groups are the same block
        ea, eu = np.tile(ea, (3, 1, 1)), np.tile(eu, (3, 1))
    if c.shape == "L":                                                # a row per (group, mode), tiled in time
        n = held(what + ", amps", amps.view(c.n_grp * c.K, c.n_t), whole(ea.reshape(c.n_grp * c.K, T_B), c.n_t, c.lead))
        return n + held(what + ", n_used", n_used.view(c.n_grp, c.n_t), whole(eu, c.n_t, c.lead))
    n = held(what + ", amps", flat(amps), whole(ea.reshape(1, -1), amps.numel()))
    return n + held(what + ", n_used", flat(n_used), whole(eu.reshape(1, -1), n_used.numel()))


MODE = [("W", t, K) for t in "AB" for K in (1, 3)] + [("G", t, K) for t in "AB" for K in (1, 2, 3)] + [("L", t, 1) for t in "AB"]


@pytest.mark.parametrize("shape,tier,K", MODE, ids=["%s-%s-K%d" % p for p in MODE])
def test_modefilter(pj, dev, shape, tier, K):
    """k_modefilter<K>.  W: the block's four groups tiled with the detectors, the C = 64 tile, 6 10^6 blocks.  G: three giant
    groups of k = 1024 (tier A) and 2048 (tier B, in place: a lane's r * n_t + t passes 2^32 inside one group) copies of a 71-row block on
    exact inputs, the C = 16 tile.  L: one group of all detectors and an empty one,
    tiled in time: r * n_t + t and ((sp - 1) * K + i) * n_t + t."""
    c = LT.modefilter(shape, tier, K)
    what = "modefilter %s %s K = %d (%d x %d, %d groups, C = %d)" % (shape, tier, K, c.n_det, c.n_t, c.n_grp, c.C)
    t0 = _begin(dev, c, what)
    m = Bufs()
    try:
        _modefilter_setup(m, c, dev)
        call_entry(pj, "pxl_tod_modefilter_f64", c.n_det, c.n_t, c.n_grp, m.grp, K, m.modes, LT.RCOND_MIN, m.d, m.w, m.out, m.amps, m.n_used)
        n = held(what, m.out, _modefilter_out_spans(c))
        assert n == c.n_det * c.n_t
        if not c.in_place:
            assert _modefilter_fit_held(what, c, m.amps, m.n_used) == c.n_grp * (K + 1) * c.n_t
            n += c.n_grp * (K + 1) * c.n_t
        _report(what, t0, dev, n)
    finally:
        _release(m)


# ================================================================================================
# toeplitz
# ================================================================================================

def _toeplitz_setup(m, c, dev):
    _filter_inputs(m, c, dev)
    rows = c.n_det if c.shape == "L" else 1
    m.kern = tiled(c.blk["kern"], 1, c.n_det * (c.lam + 1), dev)
    m.seg = torch.tensor(c.seg, dtype=I64, device=dev)
    assert m.out.data_ptr() != m.d.data_ptr() and m.out.shape == (rows, c.n_det * c.n_t // rows)


def _toeplitz_long_held(what, c, out, dev):
    """The long shape's expectation: the windows around every offset against the yardstick on the host, then -- the window's
    in-segment samples overwritten with the tiling they were not expected to match -- +0.0 outside the segments and the
    circular result tiled inside, densely."""
    x, w, kern, lam, seg = c.blk["d"], c.blk["w"], c.blk["kern"], c.lam, c.seg
    circ = to_dev(c.exp["out"], dev)
    n = 0
    for j, e in enumerate(seg):
        first, last = j == 0, j == len(seg) - 1
        win = LT.toeplitz_window(x, w, kern, e, first, last)
        same_bits(out[:, e - lam:e + lam].cpu().numpy(), win, "%s, the window at offset %d = %d" % (what, j, e))
        lo, hi = e - (0 if first else lam), e + (0 if last else lam)
        out[:, lo:hi] = circ[:, torch.arange(lo, hi, device=dev) % T_B]
        n += 2 * lam * c.n_det
    zero = np.zeros((1, 1))
    return n, held(what, out, [(0, seg[0], zero, 0), (seg[0], seg[-1], c.exp["out"], 0), (seg[-1], c.n_t, zero, 0)])


TOEP = [(s, t, lam) for t in "AB" for s in "WL" for lam in (3, 64)] + [("W", "A", 1025), ("C", "A", 3)]


@pytest.mark.parametrize("shape,tier,lam", TOEP, ids=["%s-%s-l%d" % p for p in TOEP])
def test_toeplitz(pj, dev, shape, tier, lam):
    """k_toeplitz: <128, false> at lambda = 3, <128, true> at 64, <4096, true> at 1025.  W: the block's segments, seams at the
    1280-sample tile's edges, blockIdx.x / tiles and det * (lambda + 1).  L: 200 long segments, t0, t and the offsets up to n_t.
    Tier A with wlive, tier B without."""
    c = LT.toeplitz(shape, tier, lam)
    what = "toeplitz %s %s lambda %d (%d x %d, %d segments)" % (shape, tier, lam, c.n_det, c.n_t, c.n_seg)
    shape = c.shape                                                   # a chunk case reads as a wide one
    t0 = _begin(dev, c, what)
    m = Bufs()
    try:
        _toeplitz_setup(m, c, dev)
        call_entry(pj, "pxl_tod_toeplitz_f64", c.n_det, c.n_t, c.n_seg, m.seg, lam, m.kern, m.d, m.w, m.out)
        if shape == "W":
            extra, n = 0, held(what, m.out, whole(c.exp["out"].reshape(1, -1), c.n_det * c.n_t))
        else:
            extra, n = _toeplitz_long_held(what, c, m.out, dev)
        assert n == c.n_det * c.n_t
        _report(what, t0, dev, n + extra)
    finally:
        _release(m)


# ================================================================================================
# pointing_expand
# ================================================================================================

@pytest.mark.parametrize("with_gamma", [False, True], ids=["gamma_null", "gamma"])
@pytest.mark.parametrize("shape", ["W", "L", "C"])
def test_pointing_expand(pj, dev, bound, shape, with_gamma):
    """k_pointing_expand.  W: nd = k 11 detectors on nt = 10007, N just past 2^31: `blockIdx.x % ntb` and d * nt + t, 32 GiB for each
    output.  L: 8 detectors on nt just past 2^28, the boresight tiled in time.  The block is the device's own call, held to
    pointing_ref's long double under test_gpu_pointing.py's bound."""
    c = LT.pointing(shape)
    what = "pointing_expand %s %s (%d x %d)" % (shape, "gamma" if with_gamma else "gamma null", c.n_det, c.n_t)
    shape = c.shape                                                   # a chunk case reads as a wide one
    t0 = _begin(dev, c, what)
    m = Bufs()
    try:
        qb, qd, gamma = c.blk["qb"], c.blk["qd"], c.blk["gamma"] if with_gamma else None
        sky_b, resp_b = pj.expand_pointing(to_dev(qb, dev), to_dev(qd, dev), None if gamma is None else to_dev(gamma, dev))
        sky_b, resp_b = sky_b.cpu().numpy(), resp_b.cpu().numpy()
        got = {"ra": sky_b[:, 0], "dec": sky_b[:, 1], "q": resp_b[:, 0], "u": resp_b[:, 1]}
        pos, resp = PR.worst(got, PR.expand(qb, qd, gamma, dtype=np.longdouble), None if gamma is None else np.repeat(gamma, c.t_b))
        print("%s, the block: position %.2f / %.2f, response %.2f / %.2f" % (what, pos, bound[0], resp, bound[1]))
        assert pos <= bound[0] and resp <= bound[1]
        for th in LT.THRESHOLDS:                                      # what test_large_tod_case.test_period asks of a host-made expectation
            for name, a in (("sky", sky_b), ("resp", resp_b)):
                rows_b = a.reshape(1, -1) if shape == "W" else a.reshape(c.rows, -1)
                assert all(LT.roll_differs(r, th % r.size)[0] >= 0.99 for r in rows_b), (name, th)
        if shape == "W":
            m.qbore = to_dev(qb, dev)
            m.qdet = tiled(qd, 1, 4 * c.n_det, dev)
            m.gamma = tiled(gamma, 1, c.n_det, dev) if with_gamma else None
            rows = 1
        else:
            m.qbore = tiled(qb, 1, 4 * c.n_t, dev)
            m.qdet = to_dev(qd, dev)
            m.gamma = to_dev(gamma, dev) if with_gamma else None
            rows = c.n_det
        m.sky, m.resp = sentinel(2 * c.n, dev), sentinel(2 * c.n, dev)
        call_entry(pj, "pxl_pointing_expand_f64", c.n_t, m.qbore, c.n_det, m.qdet, m.gamma, m.sky, m.resp)
        n = held(what + ", sky", m.sky.view(rows, -1), whole(sky_b.reshape(rows, -1), 2 * c.n // rows))
        n += held(what + ", resp", m.resp.view(rows, -1), whole(resp_b.reshape(rows, -1), 2 * c.n // rows))
        assert n == 4 * c.n
        _report(what, t0, dev, n)
    finally:
        _release(m)


# ================================================================================================
# the Python wrappers, once each at shape W, tier A: a given out, (D, T) weights, a prebuilt plan
# ================================================================================================

def _same_dense(a, b, what):
    """Two (1, n) Float64 device tensors have the same bits, a slab at a time."""
    a, b = a.view(I64).reshape(-1), b.view(I64).reshape(-1)
    for i in range(0, a.numel(), LT.SLAB):
        assert torch.equal(a[i:i + LT.SLAB], b[i:i + LT.SLAB]), "%s: the wrapper's bits differ from the raw call's in [%d, %d)" % (what, i, i + LT.SLAB)
    return a.numel()


@pytest.mark.parametrize("op", ["polyfilter", "modefilter", "binfilter", "toeplitz"])
def test_wrapper_gives_the_raw_calls_bits(pj, dev, op):
    """pj.polyfilter_tod (order 3), pj.modefilter_tod (K = 3), pj.binfilter_tod and pj.toeplitz_tod (lambda = 64) on the wide tier-A
    case: the same bits as the raw call in a second out, itself held to the expectation, and the fit's outputs held too."""
    c = {"polyfilter": lambda: LT.polyfilter("W", "A", 3), "modefilter": lambda: LT.modefilter("W", "A", 3),
         "binfilter": lambda: LT.binfilter("W", "A"), "toeplitz": lambda: LT.toeplitz("W", "A", 64)}[op]()
    what = "pj.%s_tod W A (%d x %d)" % (op, c.n_det, c.n_t)
    n_all = c.n_det * c.n_t
    fit_outputs = sum(n for name, n in c.big.items() if name in ("coeffs", "amps", "means", "n_used"))
    t0 = _begin(dev, c, what, extra_bytes=8 * (n_all + fit_outputs))             # the second out, and the fit's outputs the wrapper allocates
    m = Bufs()
    try:
        shape2 = (c.n_det, c.n_t)
        m.out2 = sentinel(n_all, dev).view(shape2)
        if op == "polyfilter":
            _polyfilter_setup(m, c, dev)
            call_entry(pj, "pxl_tod_polyfilter_f64", c.n_det, c.n_t, c.n_seg, m.seg, c.order, LT.RCOND_MIN, m.d, m.w, m.out, m.coeffs, m.n_used)
            res, m.co2, m.nu2 = pj.polyfilter_tod(m.d.view(shape2), c.seg, c.order, w=m.w.view(shape2), out=m.out2, rcond_min=LT.RCOND_MIN,
                                                  return_fit_info=True)
            n = _polyfilter_fit_held(what, c, m.co2, m.nu2)
            spans = _polyfilter_out_spans(c)
        elif op == "modefilter":
            _modefilter_setup(m, c, dev)
            call_entry(pj, "pxl_tod_modefilter_f64", c.n_det, c.n_t, c.n_grp, m.grp, c.K, m.modes, LT.RCOND_MIN, m.d, m.w, m.out, m.amps, m.n_used)
            res, m.co2, m.nu2 = pj.modefilter_tod(m.d.view(shape2), m.modes.view(c.n_det, c.K), w=m.w.view(shape2), grp_start=m.grp.tolist(),
                                                  out=m.out2, rcond_min=LT.RCOND_MIN, return_fit_info=True)
            n = _modefilter_fit_held(what, c, m.co2, m.nu2)
            spans = _modefilter_out_spans(c)
        elif op == "binfilter":
            _binfilter_setup(m, c, dev)
            call_entry(pj, "pxl_tod_binfilter_f64", c.n_det, c.n_t, c.n_bin, m.start, m.order, m.d, m.w, m.out, m.means, m.n_used)
            plan = pj.bin_plan(torch.from_numpy(LT._bin_index(7)).to(dev), c.n_bin)
            assert torch.equal(plan[0], m.order) and torch.equal(plan[1], m.start)
            res, m.co2, m.nu2 = pj.binfilter_tod(m.d.view(shape2), plan, w=m.w.view(shape2), out=m.out2, return_fit_info=True)
            n = _binfilter_fit_held(what, c, m.co2, m.nu2)
            spans = _binfilter_out_spans(c)
        else:
            _toeplitz_setup(m, c, dev)
            call_entry(pj, "pxl_tod_toeplitz_f64", c.n_det, c.n_t, c.n_seg, m.seg, c.lam, m.kern, m.d, m.w, m.out)
            res = pj.toeplitz_tod(m.d.view(shape2), m.kern.view(c.n_det, c.lam + 1), seg_start=c.seg, w=m.w.view(shape2), out=m.out2)
            n = 0
            spans = whole(c.exp["out"].reshape(1, -1), n_all)
        assert res.data_ptr() == m.out2.data_ptr()
        del res
        n += _same_dense(m.out, m.out2, what)
        n += held(what, flat(m.out2), spans)
        assert n >= 2 * n_all
        _report(what, t0, dev, n)
    finally:
        _release(m)
