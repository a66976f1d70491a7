"""The cases of tests/test_gpu_large_tods.py, built on the CPU alone (numpy; no device, no library): the timestream kernels
k_polyfilter, k_modefilter, k_binfilter, k_toeplitz and k_pointing_expand on (D, T) buffers whose flat element offsets
det * n_t + t pass 2^29, 2^31 and 2^32.  tests/test_large_tod_case.py shows what is claimed here without a device.

THE METHOD is technique 1 of test_gpu_second_trip.py, a checked block, tiled.  A small BLOCK of rows x T_B samples is drawn on the
host with its weights, plan, couplings or kernel; the operator's own yardstick (polyfilter_ref, modefilter_ref, binfilter_ref,
toeplitz_ref in Float64, in the device's summation order where the inputs are not exact) gives the block's expected bits; the
device tiles the block into the big arguments and EVERY element of every output of the one big call is compared, as integers,
with the tiling of the expectation.  Nothing dense is built on the host.

THE SIZES.  T_B = 10007 samples (prime: no multiple of 64, 256 or 1280).  ROWS = 21 rows for the wide shapes, 71 for the
mode filter's giant groups, 11 and 8 detectors for pointing_expand; the period P of a tiling -- the elements of one block in flat
order, rows * T_B for a wide shape, T_B along a row of a long one -- is always odd, so 2^k mod P is never 0 and an offset that
lost its high bits lands on another phase of the block.

  shape W, wide   n_t = T_B, n_det = k * rows: det * n_t crosses the thresholds, the grids reach 10^6 to 10^7 blocks.
  shape L, long   n_t = LEAD + k * T_B + TAIL with 3 detectors (tier A, n_t > 2^29: byte offsets pass 2^32 inside a row, the
                  last row passes 2^31) or 2 (tier B, n_t > 2^31: t itself, seg_start and order pass 2^31).  A tier-B row is
                  2^31 + 2^27 samples, 34 GiB per buffer, not "just past" 2^31: with two rows of 2^31 + T_B samples only the
                  last offset of seg_start and of bin_start would lie past 2^31, and no bin's positions of `order`.
  tier A          just past 2^31 elements plus one block: 16 GiB per Float64 buffer, every argument present.
  tier B          just past 2^32 elements plus one block: 32 GiB per buffer, two big buffers (the filters in place with wfit,
                  Toeplitz x and out without wlive).

  shape C, chunk  the entries launch a grid in chunks of CHUNK_BLOCKS = 2^24 - 8 blocks (one launch runs blocks * 256 mod 2^32
                  work-items; the wide tier-B bin filter and the long mode filter were the cases that found it).  The other three
                  kernels reach their second chunk on short rows: 3 rows x 33 samples for polyfilter (G = 64, four items a
                  block), 3 x 7 for Toeplitz (a block a row), 11 detectors x 3 samples for pointing_expand (a block per eight
                  detectors), tiled to just past 2^24 blocks: 0.7, 0.1 and 0.4 10^9 elements.  A Case of shape C reads as shape W.

A Case holds the host block (`blk`), the expected block (`exp`: Float64 arrays and int64 counts), the big call's sizes, the
element counts of its big buffers (`big`) and what the plan costs in bytes (`plan_bytes`, slab temporaries of the dense compare
included).  Builders are cached: a yardstick is computed once per process and never changed."""
import functools
import types

import numpy as np

import binfilter_ref as BF
import modefilter_ref as MF
import polyfilter_ref as PF
import toeplitz_ref as TR

GIB = 2 ** 30
CAP_BYTES = 96 * GIB
T_B = 10007
ROWS = 21                               # rows of a wide block: P = 210 147
ROWS_GIANT = 71                         # rows of the mode filter's giant-group block: P = 710 497
ROWS_PT_W, ROWS_PT_L = 11, 8            # detectors of pointing_expand's blocks (its group is 8 detectors)
LEAD, TAIL = 1531, 4099                 # samples of a long row before the first and after the last whole copy of the block
TOTAL = {"A": 2 ** 31, "B": 2 ** 32}
PAST = 2 ** 27                          # samples of a tier-B long row beyond 2^31: one in seventeen of its segments, bins and samples
THRESHOLDS = (2 ** 29, 2 ** 31, 2 ** 32)
SLAB = 2 ** 27                          # elements the dense compare looks at in one step (at most 2^28)
SLAB_BYTES = 8 * SLAB * 4               # its temporaries: an int64 gather of a partial period and a few masks, generously
RCOND_MIN = 1e-10
SENTINEL_BITS = 0x7ff8dead0000beef      # a NaN with a payload: what every output holds before the call
N_BIN = 300
CHUNK_BLOCKS = 2 ** 24 - 8              # PXL_CHUNK_BLOCKS of csrc/pxl_kernels.hip, which names this mirror: change both


def wide_k(tier, rows=ROWS):
    """Whole copies of a rows x T_B block that are just past the tier's total plus one block."""
    return TOTAL[tier] // (rows * T_B) + 2


def long_shape(tier):
    """(n_det, k, n_t) of a long shape: k whole copies of the block along each row, LEAD samples before and TAIL after."""
    n_det = 3 if tier == "A" else 2
    k = (TOTAL[tier] // n_det + (PAST if tier == "B" else 0)) // T_B + 2
    return n_det, k, LEAD + k * T_B + TAIL


def crossings(n_elems):
    """The thresholds a buffer of n_elems elements holds strictly inside: 0 < threshold <= n_elems - 1."""
    return [th for th in THRESHOLDS if 0 < th <= n_elems - 1]


def _case(**kw):
    c = types.SimpleNamespace(**kw)
    c.starts_tiled = c.op == "polyfilter" and c.shape == "L"            # starts are offsets into every copy of the block, after c.lead
    c.plan_bytes = 8 * sum(c.big.values()) + SLAB_BYTES
    return c


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

def draw(rows, seed, cut=0.1, nan=True, nt=T_B):
    """(d, w) as test_gpu_polyfilter.make_data draws them -- noise of rms 1 on a slow drift of amplitude 100, weights in [0.5, 2)
    with a fraction `cut` of exact zeros -- and a NaN in d under three cuts in ten."""
    rng = np.random.default_rng(seed)
    t = np.arange(nt) / nt
    d = rng.normal(size=(rows, nt)) + 100.0 * np.sin(3.0 * t + rng.uniform(0, 6, (rows, 1)))
    w = rng.uniform(0.5, 2.0, (rows, nt)) * (rng.uniform(0, 1, (rows, nt)) >= cut)
    if nan:
        d[(w == 0) & (rng.uniform(0, 1, (rows, nt)) < 0.3)] = np.nan
    return d, w


def draw_exact(rows, seed):
    """(d, w): integers in [-1024, 1024] and weights from {0, 1/2, 1, 2, -1, NaN}: every moment sum is exact in any order."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-1024, 1025, (rows, T_B)).astype(np.float64)
    w = rng.choice(np.array([0.0, 0.5, 1.0, 2.0, -1.0, np.nan]), size=(rows, T_B), p=[0.1, 0.2, 0.4, 0.2, 0.05, 0.05])
    return d, w


def tile_host(blk, m, lead=0, n=None):
    """numpy's form of the device's tiling along the last axis: big[..., t] = blk[..., (t - lead) mod p], n samples (m copies)."""
    p = blk.shape[-1]
    n = m * p if n is None else n
    return blk[..., (np.arange(n) - lead) % p]


# ---- polyfilter -----------------------------------------------------------------------------------------------------------------

POLY_W_SEG = [3, 3, 520, 1279, 1281, 2304, 2304, 3100, 3163, 4187, 4700, 5555, 6400, 7001, 7700, 8500, 9300, T_B - 6]
POLY_L_OFF = [0, 2503, 5000, 7498]      # a tile's four segments; the last ends where the next tile begins


@functools.lru_cache(maxsize=None)
def polyfilter(shape, tier, order):
    """W: the block's 17 segments (mean 588 samples: G <= 64) on every row, orders 0 and 3.  L: four segments per copy of the
    block (mean 2501: G = 256), seg_start = LEAD + i T_B + POLY_L_OFF, LEAD samples before the first and TAIL after the last are
    copied, orders 1 and 7."""
    if shape == "W":
        k, rows = wide_k(tier), ROWS
        n_det, n_t, seg, n_seg = k * rows, T_B, POLY_W_SEG, len(POLY_W_SEG) - 1
    elif shape == "C":                                                # 3 items a row, 4 items a block: the second chunk from row 22 369 622 on
        rows, n_t, seg, n_seg = 3, 33, [0, 33], 1
        k = -(-(CHUNK_BLOCKS + 16) * 4 // 3) // rows + 1
        n_det, shape = k * rows, "W"
    else:
        rows, k, n_t = long_shape(tier)
        n_det, seg, n_seg = rows, POLY_L_OFF + [T_B], 4 * k
    d, w = draw(rows, 100 + 10 * order + (shape == "L") + 2 * (tier == "B"), nt=n_t if shape == "W" else T_B)
    G = PF.group(n_t, n_seg, order)
    fit = PF.filter(d, seg, order, wfit=w, rcond_min=RCOND_MIN, lanes=None if G == 1 else G)
    n = n_det * n_t
    big = {"d": n, "w": n} if tier == "B" else {"d": n, "w": n, "out": n, "coeffs": n_det * n_seg * (order + 1), "n_used": n_det * n_seg}
    if shape == "L":
        big["seg_start"] = n_seg + 1
    return _case(op="polyfilter", shape=shape, tier=tier, order=order, rows=rows, k=k, n_det=n_det, n_t=n_t, n_seg=n_seg, seg=seg, G=G,
                 P=rows * n_t if shape == "W" else T_B, lead=0 if shape == "W" else LEAD, in_place=tier == "B",
                 blk={"d": d, "w": w}, exp={"out": fit.out, "coeffs": fit.coeffs, "n_used": fit.n_used}, big=big,
                 starts=set(seg[:-1]))


# ---- binfilter ------------------------------------------------------------------------------------------------------------------

def _bin_index(seed):
    """A scan's bin index over the block: a triangle sweep of period 997 samples over N_BIN bins, -1 at the turnarounds."""
    t = np.arange(T_B)
    ph = (t % 997) / 997.0
    az = np.where(ph < 0.5, 2 * ph, 2 - 2 * ph)
    idx = np.minimum((az * N_BIN).astype(np.int64), N_BIN - 1)
    idx[(az < 0.01) | (az > 0.99)] = -1
    return idx


def binfilter_long_plan(order_b, start_b, m, tail=0):
    """The plan of m copies of the block along a row (and `tail` samples after them in no bin), bin by bin: bin b gathers its
    samples from ALL copies, copy by copy, so the plan is the stable sort the kernel's header asks for."""
    parts = []
    for b in range(len(start_b)):                                     # the last round: the samples in no bin
        pos = order_b[start_b[b]:start_b[b + 1] if b + 1 < len(start_b) else T_B]
        parts.append((pos[None, :] + (np.arange(m) * T_B)[:, None]).reshape(-1))
    parts.append(m * T_B + np.arange(tail))
    return np.concatenate(parts).astype(np.int64), m * np.asarray(start_b, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def binfilter(shape, tier):
    """W: the block's plan, shared by all rows, random reals.  L: N_BIN bins that each gather from all k copies of the block,
    exact inputs: every moment sum is exact and fl(k b / k g) = fl(b / g), so the big call has the block's bits for any k."""
    order_b, start_b = BF.plan(_bin_index(7), N_BIN)
    if shape == "W":
        k, rows = wide_k(tier), ROWS
        n_det, n_t = k * rows, T_B
        d, w = draw(rows, 200 + (tier == "B"))
        n_plan = T_B
    else:
        rows, k, n_t = long_shape(tier)
        n_t -= LEAD                                                   # the copies start at sample 0: n_t = k T_B + TAIL
        n_det = rows
        d, w = draw_exact(rows, 210 + (tier == "B"))
        n_plan = n_t
    G = BF.group(n_t, N_BIN)
    fit = BF.filter(d, order_b, start_b, wfit=w, lanes=None if (shape == "L" or G == 1) else G)
    n = n_det * n_t
    big = {"d": n, "w": n} if tier == "B" else {"d": n, "w": n, "out": n}
    if shape == "L":
        big["order"] = n_plan
    elif tier == "A":
        big.update(means=n_det * N_BIN, n_used=n_det * N_BIN)
    first = {int(order_b[s]) for s, e in zip(start_b[:-1], start_b[1:]) if e > s}
    return _case(op="binfilter", shape=shape, tier=tier, rows=rows, k=k, n_det=n_det, n_t=n_t, n_bin=N_BIN, G=G, exact=shape == "L",
                 P=rows * T_B if shape == "W" else T_B, lead=0, in_place=tier == "B", order_b=order_b, start_b=start_b,
                 blk={"d": d, "w": w}, exp={"out": fit.out, "means": fit.means, "n_used": fit.n_used}, big=big, starts=first)


# ---- modefilter -----------------------------------------------------------------------------------------------------------------

MODE_W_GRP = [0, 5, 12, 12, ROWS]       # the block's groups, one empty; tiled with the detectors


@functools.lru_cache(maxsize=None)
def modefilter(shape, tier, n_modes):
    """W ("many"): the block's four groups tiled with the detectors, random reals: n_grp = 4 k, the C = 64 tile.  G ("giant"):
    three groups, each k copies of a 71-row block, k a power of two, exact inputs and integer couplings: every operation of the
    LDL^T scales exactly by k and the bits are the block's; n_t = T_B keeps the C = 16 tile.  L: one group of all detectors and
    one empty group, random reals, tiled in time."""
    K = n_modes
    rng = np.random.default_rng(300 + K + 10 * "WGL".index(shape) + (tier == "B"))
    lead = 0
    if shape == "W":
        k, rows = wide_k(tier), ROWS
        n_det, n_t, grp_b = k * rows, T_B, MODE_W_GRP
        n_grp = k * (len(grp_b) - 1)
        d, w = draw(rows, 310 + K + (tier == "B"))
        modes = rng.normal(size=(rows, K)) + (np.arange(K) == 0)
    elif shape == "G":
        rows, k = ROWS_GIANT, {"A": 1024, "B": 2048}[tier]
        n_det, n_t, grp_b, n_grp = 3 * k * rows, T_B, [0, rows], 3
        d, w = draw_exact(rows, 320 + K + (tier == "B"))
        modes = rng.integers(1, 4, (rows, K)).astype(np.float64) * rng.choice([-1.0, 1.0], (rows, K))
    else:
        rows, k, n_t = long_shape(tier)
        n_det, grp_b, n_grp, lead = rows, [0, rows, rows], 2, LEAD
        d, w = draw(rows, 330 + K + (tier == "B"))
        modes = rng.normal(size=(rows, K)) + 1.0
    C = MF.tile(n_t, n_grp)
    fit = MF.filter(d, modes, grp_b, wfit=w, rcond_min=RCOND_MIN, phases=256 // C)
    n = n_det * n_t
    big = {"d": n, "w": n} if tier == "B" else {"d": n, "w": n, "out": n, "amps": n_grp * K * n_t, "n_used": n_grp * n_t}
    return _case(op="modefilter", shape=shape, tier=tier, K=K, rows=rows, k=k, n_det=n_det, n_t=n_t, n_grp=n_grp, grp_b=grp_b, C=C,
                 exact=shape == "G", P=T_B if shape == "L" else rows * T_B, lead=lead, in_place=tier == "B",
                 blk={"d": d, "w": w, "modes": modes}, exp={"out": fit.out, "amps": fit.amps, "n_used": fit.n_used}, big=big,
                 starts=set())


# ---- toeplitz -------------------------------------------------------------------------------------------------------------------

TOEP_W_SEG = [3, 700, 1279, 1281, 2565, 5000, 5000, 7777, T_B - 6]      # seams one sample either side of a 1280-sample tile edge
TOEP_L_NSEG = 200


def toeplitz_instance(lam):
    """The kernel instantiation the host picks for lambda: (LMAX, SLIDE) of k_toeplitz."""
    return (128, False) if lam <= 16 else (128, True) if lam <= 128 else (1024, True) if lam <= 1024 else (4096, True)


def toeplitz_long_seg(n_t, n_seg=TOEP_L_NSEG):
    """n_seg long segments from LEAD to n_t - TAIL with seams at odd places: no multiple of the 1280-sample tile or of T_B."""
    span = n_t - LEAD - TAIL
    return [LEAD + (j * span) // n_seg + (7 * j) % 1279 * (0 < j < n_seg) for j in range(n_seg + 1)]


def toeplitz_circular(x, w, kern):
    """The block's circular result: the yardstick on three copies of the block in one segment, the middle copy kept.  A sample
    further than lambda from both ends of its segment, in a row tiled from the block, has these bits."""
    x3, w3 = np.tile(x, (1, 3)), None if w is None else np.tile(w, (1, 3))
    return TR.apply(x3, kern, [0, 3 * T_B], w3)[:, T_B:2 * T_B]


def toeplitz_window(x, w, kern, e, first, last):
    """The yardstick's values of the samples [e - lambda, e + lambda) around the segment offset e of a row tiled from the block
    (big[t] = blk[t mod T_B]): the window [e - 2 lambda, e + 2 lambda) with its seam, the segments either side at least
    2 lambda long.  first / last: e is the first / last offset, no segment on that side."""
    lam = np.shape(kern)[-1] - 1
    t = np.arange(e - 2 * lam, e + 2 * lam) % T_B
    seg = [2 * lam, 4 * lam] if first else [0, 2 * lam] if last else [0, 2 * lam, 4 * lam]
    return TR.apply(x[:, t], kern, seg, None if w is None else w[:, t])[:, lam:3 * lam]


def toeplitz_long_expect(x, w, kern, seg, n_t):
    """The dense expectation of a long row, for sizes the host can hold: +0.0 outside the segments, the circular result tiled
    inside, the windows patched in around every offset."""
    lam = np.shape(kern)[-1] - 1
    exp = np.zeros((x.shape[0], n_t))
    exp[:, seg[0]:seg[-1]] = tile_host(toeplitz_circular(x, w, kern), 0, n=n_t)[:, seg[0]:seg[-1]]
    for j, e in enumerate(seg):
        win = toeplitz_window(x, w, kern, e, j == 0, j == len(seg) - 1)
        exp[:, e - lam:e + lam] = win
    return exp


@functools.lru_cache(maxsize=None)
def toeplitz(shape, tier, lam):
    """W: the block's segments, seams at the tile's edges, a kernel per detector.  L: TOEP_L_NSEG long segments (every block of
    the kernel scans all of seg_start); exp holds the circular result, the windows come from toeplitz_window."""
    if shape == "W":
        k, rows = wide_k(tier), ROWS
        n_det, n_t, seg = k * rows, T_B, TOEP_W_SEG
    elif shape == "C":                                                # a block a row: the second chunk from row 2^24 - 8 on
        rows, n_t, seg = 3, 7, [1, 6]
        k = (CHUNK_BLOCKS + 16) // rows + 1
        n_det, shape = k * rows, "W"
    else:
        rows, k, n_t = long_shape(tier)
        n_det, seg = rows, toeplitz_long_seg(n_t)
    rng = np.random.default_rng(400 + lam + (shape == "L") + 2 * (tier == "B"))
    x, w = draw(rows, 410 + lam + (tier == "B"), cut=0.04, nt=n_t if shape == "W" else T_B)
    w[rng.uniform(0, 1, w.shape) < 0.005] = -1.0
    w[rng.uniform(0, 1, w.shape) < 0.005] = np.nan
    if tier == "B":
        w = None
        x = np.nan_to_num(x, nan=0.5)                                 # no cut to hide a NaN under
    kern = rng.normal(size=(rows, lam + 1)) / (1.0 + np.arange(lam + 1)) ** 0.5
    out = TR.apply(x, kern, seg, w) if shape == "W" else toeplitz_circular(x, w, kern)
    n = n_det * n_t
    big = {"x": n, "out": n} if tier == "B" else {"x": n, "w": n, "out": n}
    big["kern"] = n_det * (lam + 1)
    return _case(op="toeplitz", shape=shape, tier=tier, lam=lam, rows=rows, k=k, n_det=n_det, n_t=n_t, seg=seg, n_seg=len(seg) - 1,
                 P=rows * n_t if shape == "W" else T_B, lead=0, in_place=False, blk={"d": x, "w": w, "kern": kern}, exp={"out": out},
                 big=big, starts=set(seg[:-1]) if shape == "W" else set(seg))


# ---- pointing_expand ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pointing(shape):
    """W: nd = k * 11 detectors, nt = T_B, N just past 2^31 samples: 32 GiB for each of the two double2 outputs.  L: nd = 8,
    nt = k T_B + TAIL just past 2^28, the boresight tiled in time: d * nt passes 2^31 and the byte offsets pass 2^32 inside the first
    row.  Tier B (128 GiB of outputs) does not fit and is left out.  The expectation is the device's own call on the block."""
    import pointing_ref as ref
    rng = np.random.default_rng(500 + (shape == "L"))
    t_b = T_B
    if shape == "W":
        rows, k = ROWS_PT_W, wide_k("A", ROWS_PT_W)
        nd, nt = k * rows, T_B
    elif shape == "C":                                                # a block per eight detectors: the second chunk from detector 2^27 - 64 on
        rows, nt, t_b = ROWS_PT_W, 3, 3
        k = (CHUNK_BLOCKS + 16) * 8 // rows + 1
        nd, shape = k * rows, "W"
    else:
        rows, k = ROWS_PT_L, 2 ** 28 // T_B + 2
        nd, nt = rows, k * T_B + TAIL
    qb = np.concatenate((ref.random_quats(rng, T_B - 2000), ref.polar_quats(rng, 2000)))[rng.permutation(T_B)][:t_b]
    qd = ref.random_quats(rng, rows)
    gamma = rng.uniform(0.1, 1.0, rows)
    n = nd * nt
    return _case(op="pointing", shape=shape, tier="A", rows=rows, k=k, n_det=nd, n_t=nt, t_b=t_b, P=rows * t_b if shape == "W" else T_B, lead=0,
                 blk={"qb": qb, "qd": qd, "gamma": gamma}, exp={}, big={"sky": 2 * n, "resp": 2 * n, "qbore": 4 * nt}, starts=set(),
                 n=n)


def all_cases():
    """Every case the device tests run, as (builder, arguments)."""
    out = []
    for tier in "AB":
        out += [(polyfilter, ("W", tier, o)) for o in (0, 3)] + [(polyfilter, ("L", tier, o)) for o in (1, 7)]
        out += [(binfilter, (s, tier)) for s in "WL"]
        out += [(modefilter, ("W", tier, K)) for K in (1, 3)] + [(modefilter, ("L", tier, 1))]
        out += [(toeplitz, (s, tier, lam)) for s in "WL" for lam in (3, 64)]
    out += [(modefilter, ("G", tier, K)) for tier in "AB" for K in (1, 2, 3)]
    out += [(toeplitz, ("W", "A", 1025))]
    out += [(pointing, (s,)) for s in "WL"]
    return out


def chunk_cases():
    """The cases of shape C: a second chunk of blocks for the three kernels the big cases leave in one."""
    return [(polyfilter, ("C", "A", 0)), (toeplitz, ("C", "A", 3)), (pointing, ("C",))]


def roll_differs(a, s):
    """(the fraction of the elements of the flat Float64 or int64 array whose bits differ from those s places on, the same over the
    elements that are not all-zero bits both before and after the roll)."""
    a = np.ascontiguousarray(a).reshape(-1).view(np.int64)
    r = np.roll(a, s)
    either = (a != 0) | (r != 0)
    return float((a != r).mean()), float((a != r)[either].mean()) if either.any() else 1.0


def case_id(builder, args):
    return "-".join([builder.__wrapped__.__name__] + [str(a) for a in args])
