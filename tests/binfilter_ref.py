"""The binned-template filter in numpy, in three forms: in Float64 with every sum sequential in plan order, in
np.longdouble, and in Float64 in the device's order -- lanes=G: lane l adds the live positions l, l + G, ... of an item in order from
+0.0 and fit_ref.tree joins the lanes, 256 lanes as four wavefronts, (s0 + s1) + (s2 + s3) -- which the device must match to the bit.
All follow include/pixell_hip.h's definition operation for operation (numpy never fuses a product into a sum).

filter(d, order, bin_start, wfit=None, dtype=np.float64, lanes=None) -> Fit(out, means, n_used): out (D, T), means and n_used (D, n_bin).
plan(index, n_bin) -> (order, bin_start): pj.bin_plan in numpy.  group(n_t, n_bin): the host's G."""
import collections

import numpy as np

import fit_ref

Fit = collections.namedtuple("Fit", "out means n_used")


def group(n_t, n_bin):
    """The number of lanes G that own one (detector, bin): the host's rule, from n_t and n_bin alone."""
    mean = n_t // max(n_bin, 1)
    if mean >= 1024:
        return 256
    g = 1
    while g < 64 and g < mean:
        g *= 2
    return g


def plan(index, n_bin):
    """(order, bin_start): the stable argsort of the index with every value outside [0, n_bin) set to n_bin, and the number of
    samples with a key below b for b = 0 .. n_bin."""
    index = np.asarray(index, dtype=np.int64)
    key = np.where((index >= 0) & (index < n_bin), index, n_bin)
    order = np.argsort(key, kind="stable").astype(np.int64)
    bin_start = np.array([int((key < b).sum()) for b in range(n_bin + 1)], dtype=np.int64)
    return order, bin_start


def _sum(terms, live, lanes, ft):
    """The sum of the live terms from +0.0: in order (lanes None), or in the device's order."""
    if lanes is None:
        s = ft(0.0)
        for v in terms[live]:
            s = s + v
        return s
    rows = -(-len(terms) // lanes)
    t = np.zeros(rows * lanes)
    t[:len(terms)] = np.where(live, terms, 0.0)                # +0.0 for a term that is not live changes no bit of a sum from +0.0
    acc = np.zeros(lanes)
    for row in t.reshape(rows, lanes):
        acc = acc + row
    if lanes == 256:
        s = [fit_ref.tree(acc[k * 64:(k + 1) * 64]) for k in range(4)]
        return (s[0] + s[1]) + (s[2] + s[3])
    return fit_ref.tree(acc)


def filter(d, order, bin_start, wfit=None, dtype=np.float64, lanes=None):
    ft = dtype
    assert lanes is None or dtype is np.float64
    d = np.asarray(d, dtype=np.float64)
    nd, nt = d.shape
    order = np.asarray(order, dtype=np.int64)
    # the device's lanes stride over POSITIONS, skipped ones included: keep them, as terms that are not live
    spans = fit_ref.clamp(bin_start, nt)
    out = d.astype(ft)
    means = np.zeros((nd, len(spans)), dtype=ft)
    n_used = np.zeros((nd, len(spans)), dtype=np.int64)
    one = ft(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for b, (lo, hi) in enumerate(spans):
            pos = order[lo:hi]
            inside = (pos >= 0) & (pos < nt)
            t = np.where(inside, pos, 0)
            for det in range(nd):
                w = np.ones(len(t), dtype=ft) if wfit is None else np.asarray(wfit[det, t]).astype(ft)
                dv = d[det, t].astype(ft)
                live = inside & (w > 0)
                wp = w * one
                g00 = _sum(np.where(live, wp * one, 0), live, lanes, ft)
                b0 = _sum(np.where(live, wp * np.where(live, dv, 0), 0), live, lanes, ft)
                if not g00 > ft(0.0) * g00:
                    continue
                c = b0 / g00
                means[det, b], n_used[det, b] = c, 1
                out[det, t[inside]] = dv[inside] - c * one
    return Fit(out, means, n_used)
