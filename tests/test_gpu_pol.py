"""The polarised pointing matrix on the device: pj.sample_pol, pj.scatter_pol, pj.scatter_pol_weights and the
four pxl_*_car_pol_* entries.

Forward: BIT-EXACT against (s[0] + q * s[1]) + u * s[2] formed in numpy from the device's own scalar samples s.
Transpose: against the device's scalar scatter of the products t_c formed in numpy (pol_ref.terms), and against the numpy
yardstick tests/pol_ref.py: a pixel that takes at most one non-zero term must have the same BITS, every other pixel is held to
k * 2^-52 * S (scatter_ref's derivation: the order of the atomic adds is unspecified), order 3 through F^T to
scatter_cubic_ref.composite_bound.  Two device calls are never asserted bit-equal beyond that.  Each check prints its worst
error / bound."""
import ctypes as C

import numpy as np
import pytest

import pol_ref as P
import scatter_cubic_ref as T
import scatter_ref as R
import spline_ref as SR
import tap_ref
from conftest import DEG

torch = pytest.importorskip("torch")
import gpu_support
from gpu_support import dev, edge_points, same_bits, to_dev
pytestmark = pytest.mark.gpu

# the points one block takes per trip: blockDim.x (256) times the kernel's points per lane
CHUNK = {("sample", 1): 512,          # k_sample_pol_bilinear: PXL_PSUNR = 2
         ("sample", 3): 256,          # k_sample_pol_cubic: one point per lane
         ("scatter", 1): 1024,        # k_scatter_pol_bilinear<3|6>: PXL_SUNR = 4
         ("scatter", 3): 512}         # k_scatter_pol_cubic<3|6>: PXL_CUNR = 2
LD = np.longdouble
MODES = [(1, False), (3, True), (3, False)]          # (order, prefiltered)


def _geometries(pj):
    return tap_ref.geometries(pj, ("cc_360x181", "box_80x40", "cc_1024x513", "box_4x4", "box_5x7", "box_2x2"))


def _geoms(order):
    return ["cc_360x181", "box_80x40"] + (["box_2x2"] if order == 1 else ["box_4x4", "box_5x7"])


CASES = [(o, p, g) for o, p in MODES for g in _geoms(o)]


def _combine(s, resp):
    """(s[0] + q * s[1]) + u * s[2] on the host: separate numpy operations, one rounding each."""
    with np.errstate(invalid="ignore", over="ignore"):
        return P.combine(np.asarray(s), resp)


# ---- 1. forward: bit-exact against the scalar samplers -------------------------------------------------------------------------
def _special_map(shape, seed):
    nx, ny = shape
    rng = np.random.default_rng(seed)
    m = rng.normal(size=(3, ny, nx))
    flat = m.reshape(3, -1)
    for c, vals in enumerate(([np.nan, -0.0, np.inf], [-np.inf, -0.0, 1e300], [np.nan, -0.0, -1e-310])):
        at = rng.permutation(nx * ny)[:max(3, nx * ny // 40)]
        flat[c, at] = np.resize(vals, len(at))
    return m


@pytest.mark.parametrize("order,prefiltered,geom", CASES)
def test_forward_is_bit_exact(pj, O, dev, order, prefiltered, geom):
    """pj.sample_pol against the numpy combination of pj.sample's three planes, bit patterns compared: random points, the seam,
    the pole rows, pixel edges, outside a box, NaN and Inf coordinates, NaN in resp; an ordinary map, then one with NaN, +-Inf,
    -0.0, huge and subnormal pixels."""
    shape, wcs = _geometries(pj)[geom]
    n = 20011                                                        # 40 blocks of k_sample_pol_bilinear, 79 of the cubic kernel, the last partial
    sky = edge_points(O, wcs, shape, n, 5, False)
    sky[-6:] = [[np.nan, 0.1], [0.1, np.nan], [np.inf, 0.0], [0.0, -np.inf], [np.nan, np.nan], [-np.inf, np.inf]]
    resp = np.random.default_rng(6).normal(size=(n, 2))
    resp[100] = [np.nan, 1.0]; resp[101] = [0.5, np.nan]; resp[102] = [np.inf, -0.0]; resp[103] = [0.0, 0.0]
    dsky, dresp = to_dev(sky, dev), to_dev(resp, dev)
    for kind, m in (("ordinary", np.random.default_rng(7).normal(size=(3, shape[1], shape[0]))), ("special", _special_map(shape, 8))):
        em = pj.Enmap(to_dev(m, dev), wcs)
        s = pj.sample(em, dsky, order=order, prefiltered=prefiltered).cpu().numpy()
        got = pj.sample_pol(em, dsky, dresp, order=order, prefiltered=prefiltered)
        assert tuple(got.shape) == (n,) and got.dtype == torch.float64
        got = got.cpu().numpy()
        want = _combine(s, resp)
        same_bits(got, want, "%s order %d %s" % (geom, order, kind))
        assert np.isnan(got[-6:]).all() and np.isnan(got[100]) and np.isnan(got[101])
        if kind == "ordinary":
            live = np.isfinite(got) & (got != 0)
            print("%s order %d: %d of %d values finite and not zero" % (geom, order, int(live.sum()), n))
            assert live.sum() > n // 8
            if order == 1:
                same_bits(got, P.sample(O, wcs, shape, m, sky, resp), "%s against the oracle's sampler" % geom)


def test_forward_row_strips(pj, O, dev):
    """src_rows strips of the 360 x 181 map at order 1, points whose cell a strip boundary cuts among them: the scalar sampler on
    the same strip, combined on the host, bit for bit, and the oracle's sampler on that strip; an empty strip gives zeros."""
    shape, wcs = _geometries(pj)["cc_360x181"]
    nx, ny = shape
    n = 6000
    sky = edge_points(O, wcs, shape, n, 9, False)
    rng = np.random.default_rng(10)
    cut = np.stack([rng.uniform(1, nx, 600), np.where(np.arange(600) % 2 == 0, rng.uniform(60, 61, 600), rng.uniform(120, 121, 600))], axis=1)
    sky[2000:2600] = O.pix2sky(wcs, cut, O.WRAP_NONE)
    idx, _w = R.taps(O, wcs, shape, sky, 60, 60)
    dropped = (idx[2000:2600] < 0).sum(axis=1)
    assert (dropped == 2).all(), "the strip [60, 120) holds one row of each of these cells"
    resp = rng.normal(size=(n, 2))
    m = rng.normal(size=(3, ny, nx))
    dsky, dresp = to_dev(sky, dev), to_dev(resp, dev)
    for row0, nrows in ((0, 60), (60, 60), (120, 61), (90, 0)):
        strip = pj.Enmap(to_dev(m[:, row0:row0 + nrows], dev), wcs)
        s = pj.sample_bilinear(strip, dsky, src_rows=(row0, nrows), full_shape=shape).cpu().numpy()
        got = pj.sample_pol(strip, dsky, dresp, src_rows=(row0, nrows), full_shape=shape).cpu().numpy()
        same_bits(got, _combine(s, resp), "strip [%d, %d)" % (row0, row0 + nrows))
        same_bits(got, P.sample(O, wcs, shape, m[:, row0:row0 + nrows], sky, resp, 1, False, row0, nrows), "strip against the oracle")
        if nrows == 0:
            assert not got.any()


# ---- 2. transpose against the scalar scatter and the yardstick -----------------------------------------------------------------
def _dev_scatter(pj, dev, mode, vals, sky, resp, shape, wcs, out0=None, **kw):
    fn = pj.scatter_pol_weights if mode else pj.scatter_pol
    out = None if out0 is None else to_dev(out0, dev)
    res = fn(to_dev(vals, dev), to_dev(sky, dev), to_dev(resp, dev), shape, wcs, out=out, **kw)
    assert isinstance(res, pj.Enmap)
    if out is not None:
        assert res.data.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    got = res.data.cpu().numpy()
    assert got.shape[0] == (6 if mode else 3) and got.ndim == 3
    return got


def _dev_scalar(pj, dev, t, sky, shape, wcs, order, prefiltered, out0=None, window=None):
    """The composition: the scalar scatter of the (3 or 6, N) products formed on the host."""
    out = None if out0 is None else to_dev(out0, dev)
    if window is not None:
        res = pj.scatter_bilinear(to_dev(t, dev), to_dev(sky, dev), shape, wcs, out=out, src_rows=window, full_shape=shape)
    else:
        res = pj.scatter(to_dev(t, dev), to_dev(sky, dev), shape, wcs, order=order, out=out, prefiltered=prefiltered)
    torch.cuda.synchronize()
    return res.data.cpu().numpy()


def _held_accumulating(pj, O, dev, shape, wcs, sky, vals, resp, order, mode, what, window=None, seed=3):
    """An accumulating call (order 1, or E^T) into a random map, against the yardstick and the scalar scatter.  Returns what the
    yardstick gave and the device's map."""
    row0, nrows = (0, shape[1]) if window is None else window
    nplanes = 6 if mode else 3
    out0 = gpu_support.out0(nplanes, nrows, shape[0], seed)
    wkw = {} if window is None else {"row0": row0, "nrows": nrows}
    ref, k, S = P.scatter(O, wcs, shape, sky, vals, resp, order, mode, out=out0, **wkw)
    kw = {"order": order, "prefiltered": order == 3}
    if window is not None:
        kw.update(src_rows=window, full_shape=shape)
    got = _dev_scatter(pj, dev, mode, vals, sky, resp, shape, wcs, out0, **kw)
    R.held(got, ref, k, S, what + " against the yardstick")
    scalar = _dev_scalar(pj, dev, P.terms(vals, resp, mode), sky, shape, wcs, order, order == 3, out0, window)
    R.held(got, scalar, k, S, what + " against the scalar scatter")
    single = P.nonzero_terms(O, wcs, shape, sky, vals, resp, order, mode, **wkw) <= 1
    for other, name in ((ref, "the yardstick"), (scalar, "the scalar scatter")):
        nan = np.isnan(other[single])
        assert np.array_equal(got[single].view(np.int64)[~nan], other[single].view(np.int64)[~nan]), \
            "%s: a pixel with at most one non-zero term differs in bits from %s" % (what, name)
    idle = k == 1
    assert np.array_equal(got[idle].view(np.int64), out0[idle].view(np.int64)), what + ": a pixel that receives nothing changed"
    return ref, k, S, got, out0, int(single.sum()), int(idle.sum())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("order,prefiltered,geom", CASES)
def test_transpose_against_the_scalar_scatter(pj, O, dev, order, prefiltered, geom, mode):
    shape, wcs = _geometries(pj)[geom]
    n = 20011
    sky = edge_points(O, wcs, shape, n, 12, False)
    sky[-3:] = [[np.nan, 0.1], [0.2, np.inf], [-np.inf, np.nan]]
    rng = np.random.default_rng(13 + mode)
    resp = rng.normal(size=(n, 2))
    vals = rng.normal(size=n)
    resp[200] = [0.0, 1.5]; vals[201] = 0.0                        # zero terms still add, and change nothing
    what = "%s order %d%s mode %d" % (geom, order, "" if prefiltered or order == 1 else " with F^T", mode)
    if order == 1 or prefiltered:
        ref, k, S, got, out0, single, idle = _held_accumulating(pj, O, dev, shape, wcs, sky, vals, resp, order, mode, what)
        print("%s: %d pixels with at most one non-zero term, %d untouched, max k = %d" % (what, single, idle, int(k.max())))
        if geom == "cc_360x181":
            assert idle > 0 and single > idle, "pixels left alone and pixels with one term exist on the sparse map"
        # a fresh map is a map of zeros
        fresh = _dev_scatter(pj, dev, mode, vals, sky, resp, shape, wcs, order=order, prefiltered=prefiltered)
        r0, k0, S0 = P.scatter(O, wcs, shape, sky, vals, resp, order, mode)
        R.held(fresh, r0, k0, S0, what + ", fresh map")
        return
    per = bool(O.is_periodic(wcs, shape[0]))
    ptd, g, k, S = P.scatter_full(O, wcs, shape, sky, vals, resp, 3, mode)
    cb = T.composite_bound(g, k, S, per)
    got = _dev_scatter(pj, dev, mode, vals, sky, resp, shape, wcs, order=3)
    scalar = _dev_scalar(pj, dev, P.terms(vals, resp, mode), sky, shape, wcs, 3, False)
    np_ = got.shape[0]
    for other, name in ((ptd, "the yardstick"), (scalar, "the scalar scatter")):
        err = np.abs(got - other).reshape(np_, -1).max(axis=1)
        print("%s against %s: worst error / composite bound = %.3g" % (what, name, float((err / cb).max())))
        assert np.all(err <= cb), name
    # a given map has the result added to it
    out0 = gpu_support.out0(np_, shape[1], shape[0], 4)
    acc = _dev_scatter(pj, dev, mode, vals, sky, resp, shape, wcs, out0, order=3)
    assert np.all(np.abs(acc - (out0 + ptd)).reshape(np_, -1).max(axis=1) <= cb + SR.EPS * np.abs(out0 + ptd).max())


def test_transpose_row_strips(pj, O, dev):
    """Order 1 into declination strips of the 360 x 181 map, both modes: each strip against the yardstick and the scalar scatter
    of the same window."""
    shape, wcs = _geometries(pj)["cc_360x181"]
    n = 20000
    sky = edge_points(O, wcs, shape, n, 14, False)
    rng = np.random.default_rng(15)
    resp, vals = rng.normal(size=(n, 2)), rng.normal(size=n)
    for mode in (0, 1):
        for window in ((0, 60), (60, 60), (120, 61)):
            _held_accumulating(pj, O, dev, shape, wcs, sky, vals, resp, 1, mode, "strip %s mode %d" % (window, mode), window=window)


# ---- 3. batch sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 3])
def test_batch_sizes(pj, O, dev, order):
    """n = 0, 1, chunk - 1, chunk, chunk + 1 for each of the four kernels (both instantiations of the scatters)."""
    shape, wcs = _geometries(pj)["cc_360x181"]
    m = np.random.default_rng(16).normal(size=(3, shape[1], shape[0]))
    em = pj.Enmap(to_dev(m, dev), wcs)
    sizes = {0, 1}
    for kind in ("sample", "scatter"):
        c = CHUNK[(kind, order)]
        sizes |= {c - 1, c, c + 1}
    for n in sorted(sizes):
        sky = R.sphere_points(n, n + 1)
        rng = np.random.default_rng(n)
        resp, vals = rng.normal(size=(n, 2)), rng.normal(size=n)
        dsky, dresp = to_dev(sky, dev).reshape(-1, 2), to_dev(resp, dev).reshape(-1, 2)
        got = pj.sample_pol(em, dsky, dresp, order=order, prefiltered=order == 3)
        assert tuple(got.shape) == (n,)
        s = pj.sample(em, dsky, order=order, prefiltered=order == 3).cpu().numpy()
        same_bits(got.cpu().numpy(), _combine(s, resp), "sample_pol order %d n = %d" % (order, n))
        for mode in (0, 1):
            ref, k, S, dmap, out0, _s, _i = _held_accumulating(pj, O, dev, shape, wcs, sky.reshape(-1, 2), vals, resp, order, mode,
                                                              "scatter order %d mode %d n = %d" % (order, mode, n), seed=n)
            if n == 0:
                assert np.array_equal(dmap.view(np.int64), out0.view(np.int64))
            else:
                assert (k > 1).any()


# ---- 4. contention ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("order", [1, 3])
def test_contention_in_one_cell(pj, O, dev, order, mode):
    shape, wcs = _geometries(pj)["cc_360x181"]
    n = 10 ** 5
    rng = np.random.default_rng(17 + order)
    pix = np.stack([rng.uniform(100.001, 100.999, n), rng.uniform(50.001, 50.999, n)], axis=1)
    sky = O.pix2sky(wcs, pix, O.WRAP_NONE)
    resp, vals = rng.normal(size=(n, 2)), rng.normal(size=n) + 1.0
    ref, k, S, got, out0, _s, _i = _held_accumulating(pj, O, dev, shape, wcs, sky, vals, resp, order, mode,
                                                      "one cell order %d mode %d" % (order, mode))
    taps = 4 if order == 1 else 16
    assert int((k > 1).sum()) == taps * (6 if mode else 3) and int(k.max()) == n + 1


# ---- 5. a NaN value -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("order", [1, 3])
def test_nan_value_reaches_exactly_its_taps_in_every_plane(pj, O, dev, order, mode):
    """One NaN value at a pixel centre among finite ones: its 4 or 16 taps become NaN in all three or six planes, zero weights
    included (q * NaN = NaN), and no other pixel does."""
    shape, wcs = _geometries(pj)["cc_360x181"]
    nx = shape[0]
    rng = np.random.default_rng(18)
    pix = np.stack([rng.uniform(2, nx - 1, 4000), rng.uniform(2, shape[1] - 1, 4000)], axis=1)
    pix[1234] = [200.0, 77.0]
    sky = O.pix2sky(wcs, pix, O.WRAP_NONE)
    resp, vals = rng.normal(size=(4000, 2)), rng.normal(size=4000)
    vals[1234] = np.nan
    idx, w = (R.taps if order == 1 else T.taps)(O, wcs, shape, sky)
    cell = sorted(set(idx[1234].tolist()))
    assert len(cell) == (4 if order == 1 else 16) and (w[1234] == 0).any(), "a pixel centre has zero-weight taps"
    ref, k, S, got, out0, _s, _i = _held_accumulating(pj, O, dev, shape, wcs, sky, vals, resp, order, mode, "NaN value order %d mode %d" % (order, mode))
    for c in range(got.shape[0]):
        assert sorted(np.flatnonzero(np.isnan(got[c])).tolist()) == cell, "plane %d" % c


# ---- 6. adjoint identity on the device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,geom", [(1, "cc_360x181"), (1, "box_80x40")] + [(3, g) for g in T.COMPOSITE])
def test_adjoint_identity(pj, O, dev, order, geom):
    """|<P_pol m, d> - <m, P_pol^T d>| <= bound, P_pol = pj.sample_pol and P_pol^T = pj.scatter_pol of the same order, dot
    products in long double.  The bound is the scalar tests' bound applied plane by plane, plus the combination's own roundings.

    With s_c = P m_c (the scalar sampler, which sample_pol combines bit for bit) and t_c the products pol_ref.terms forms from
    d (t_0 = d, t_1 = fl(q d), t_2 = fl(u d): what scatter_pol adds, bit for bit),
        <P_pol m, d> - <m, P_pol^T d>  =  [sum_k d_k out_k - sum_c <s_c, t_c>]  +  sum_c [<s_c, t_c> - <m_c, P^T t_c>].
    The second bracket is three scalar identities with t_c as the data.  Order 1: tests/test_gpu_scatter.py's
    2^-53 sum_p |m_p| S_p (8 + 2 k_p) per plane, k and S the yardstick's for that plane's products (scatter_ref.adjoint_gap).
    Order 3: tests/test_gpu_scatter_cubic.py's sum_k |t_ck| spline_ref.bound(m_c) + sum_p |m_cp| composite_bound_c.
    The first bracket is rounding alone: out_k = fl(fl(s_0 + fl(q s_1)) + fl(u s_2)) is within 2^-53 (2|s_0| + 3|q s_1| +
    2|u s_2|) of s_0 + q s_1 + u s_2 to first order, and s_c fl(r d) within 2^-53 |s_c r d| of s_c r d: at most four roundings
    on any summand, a fifth allowed for the second-order terms: 5 * 2^-53 sum_k |d_k| (|s_0| + |q s_1| + |u s_2|)
    (pol_ref.forward_rounding).  Dropping the responses from the forward misses the bound, so the test sees q and u."""
    if order == 1:
        shape, wcs = _geometries(pj)[geom]
        sky = np.concatenate([R.sphere_points(20000, 3), R.box_points(O, wcs, shape, 20000, 4)])
    else:
        shape, wcs, sky, _d2, _m2 = T.composite_case(pj, O, geom)
    rng = np.random.default_rng(len(geom) + order)
    n = sky.shape[0]
    m = rng.normal(size=(3, shape[1], shape[0]))
    d = rng.normal(size=n)
    resp = rng.normal(size=(n, 2))
    dsky, dresp = to_dev(sky, dev), to_dev(resp, dev)
    em = pj.Enmap(to_dev(m, dev), wcs)
    pm = pj.sample_pol(em, dsky, dresp, order=order).cpu().numpy()
    s = pj.sample(em, dsky, order=order).cpu().numpy()
    ptd = pj.scatter_pol(to_dev(d, dev), dsky, dresp, shape, wcs, order=order).data.cpu().numpy()
    assert np.isfinite(pm).all() and np.isfinite(ptd).all()
    t = P.terms(d, resp)
    ref, g, k, S = P.scatter_full(O, wcs, shape, sky, d, resp, order)
    if order == 1:
        R.held(ptd, ref, k, S, "P_pol^T d %s" % geom)
        planes = float(2.0 ** -53 * np.sum(np.abs(m).astype(LD) * S.astype(LD) * (8 + 2 * k).astype(LD)))
    else:
        cb = T.composite_bound(g, k, S, bool(O.is_periodic(wcs, shape[0])))
        assert np.all(np.abs(ptd - ref).reshape(3, -1).max(axis=1) <= cb)
        planes = float(np.sum(np.abs(t).sum(axis=1) * SR.bound(m)) + np.sum(np.abs(m).reshape(3, -1).sum(axis=1) * cb))
    bound = planes + P.forward_rounding(s, resp, d)
    rhs = np.sum(m.astype(LD) * ptd.astype(LD))
    gap = float(abs(np.sum(pm.astype(LD) * d.astype(LD)) - rhs))
    miss = float(abs(np.sum(s[0].astype(LD) * d.astype(LD)) - rhs))
    scale = float(np.sum(np.abs(pm * d)))
    print("%s order %d: |<Pm,d> - <m,PTd>| = %.3g, bound %.3g, without the responses %.3g (sum |Pm d| = %.3g)" % (geom, order, gap, bound, miss, scale))
    assert bound > 0 and gap <= bound
    assert miss > bound and miss > 1e-4 * scale, "the forward without q and u passes: the test shows nothing"


# ---- 7. raw ABI and the wrappers' refusals ---------------------------------------------------------------------------------------------
def test_einval_leaves_every_buffer_untouched(pj, dev):
    lib = pj.load_library()
    L = pj._lib
    shape, wcs = _geometries(pj)["cc_360x181"]
    w = wcs.to_struct()
    n = 2000
    dst = torch.full((6, 181, 360), -3.5, dtype=torch.float64, device=dev)
    src = torch.full((3, 181, 360), 1.25, dtype=torch.float64, device=dev)
    sky = torch.full((n, 2), 0.25, dtype=torch.float64, device=dev)         # on the map: a call that ran would add
    resp = torch.full((n, 2), 0.75, dtype=torch.float64, device=dev)
    vals = torch.full((n,), 1.5, dtype=torch.float64, device=dev)
    out = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    P_ = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    W = C.byref(w)
    shp = L.shape_arr((360, 181, 3))
    sb, sc = lib.pxl_scatter_car_pol_bilinear_f64, lib.pxl_scatter_car_pol_cubic_f64
    fb, fc = lib.pxl_sample_car_pol_bilinear_f64, lib.pxl_sample_car_pol_cubic_f64
    for nc in (1, 2, 4, 6):                                                                   # shape[2] != 3
        bad = L.shape_arr((360, 181, nc))
        assert sb(W, bad, P_(dst), 0, 181, n, P_(sky), P_(resp), P_(vals), 0, None) == -22 and "3 components" in L.last_error()
        assert sc(W, bad, P_(dst), n, P_(sky), P_(resp), P_(vals), 0, None) == -22 and "3 components" in L.last_error()
        assert fb(W, bad, P_(src), 0, 181, n, P_(sky), P_(resp), P_(out), None) == -22 and "3 components" in L.last_error()
        assert fc(W, bad, P_(src), n, P_(sky), P_(resp), P_(out), None) == -22 and "3 components" in L.last_error()
    for mode in (-1, 2, 3, 6):                                                                # a bad mode
        assert sb(W, shp, P_(dst), 0, 181, n, P_(sky), P_(resp), P_(vals), mode, None) == -22 and "mode" in L.last_error()
        assert sc(W, shp, P_(dst), n, P_(sky), P_(resp), P_(vals), mode, None) == -22 and "mode" in L.last_error()
    bad_scatter = [
        (None, shp, P_(dst), n, P_(sky), P_(resp), P_(vals)), (W, None, P_(dst), n, P_(sky), P_(resp), P_(vals)),
        (W, shp, P_(dst), -1, P_(sky), P_(resp), P_(vals)),                                   # n < 0
        (W, shp, None, n, P_(sky), P_(resp), P_(vals)), (W, shp, P_(dst), n, None, P_(resp), P_(vals)),   # null pointers with n > 0
        (W, shp, P_(dst), n, P_(sky), None, P_(vals)), (W, shp, P_(dst), n, P_(sky), P_(resp), None),
        (W, shp, P_(dst), n - 1, P_(sky, 8), P_(resp), P_(vals)),                             # a 2xN batch not 16-byte aligned
        (W, shp, P_(dst), n - 1, P_(sky), P_(resp, 8), P_(vals)),
        (W, shp, P_(dst), n, P_(sky), P_(dst, 16 * 3000), P_(vals)),                          # dst overlaps resp
        (W, shp, P_(dst), n, P_(dst, 16 * 3000), P_(resp), P_(vals)),                         # dst overlaps the points
        (W, shp, P_(dst), n, P_(sky), P_(resp), P_(dst, 8 * 1000)),                           # dst overlaps vals
    ]
    for a in bad_scatter:
        for mode in (0, 1):
            assert sb(*a[:3], 0, 181, *a[3:], mode, None) == -22, a
            assert L.last_error()
            assert sc(*a, mode, None) == -22, a
            assert L.last_error()
    # the sixth plane exists only in weights mode: resp just past three planes is clear of a signal call's dst
    past3 = P_(dst, 8 * 3 * 181 * 360)
    assert sb(W, shp, P_(dst), 0, 181, n, P_(sky), past3, P_(vals), 1, None) == -22
    assert sc(W, shp, P_(dst), n, P_(sky), past3, P_(vals), 1, None) == -22
    assert sb(W, shp, P_(dst), -1, 10, n, P_(sky), P_(resp), P_(vals), 0, None) == -22        # window outside [0, ny]
    assert sb(W, shp, P_(dst), 100, 82, n, P_(sky), P_(resp), P_(vals), 0, None) == -22
    assert sc(W, L.shape_arr((3, 181, 3)), P_(dst), n, P_(sky), P_(resp), P_(vals), 0, None) == -22   # nx < 4
    bad_sample = [
        (None, shp, P_(src), n, P_(sky), P_(resp), P_(out)), (W, None, P_(src), n, P_(sky), P_(resp), P_(out)),
        (W, shp, P_(src), -1, P_(sky), P_(resp), P_(out)), (W, shp, None, n, P_(sky), P_(resp), P_(out)),
        (W, shp, P_(src), n, None, P_(resp), P_(out)), (W, shp, P_(src), n, P_(sky), None, P_(out)),
        (W, shp, P_(src), n, P_(sky), P_(resp), None), (W, shp, P_(src), n - 1, P_(sky), P_(resp, 8), P_(out)),
        (W, shp, P_(src), n - 1, P_(sky, 8), P_(resp), P_(out)),
    ]
    for a in bad_sample:
        assert fb(*a[:3], 0, 181, *a[3:], None) == -22, a
        assert L.last_error()
        assert fc(*a, None) == -22, a
        assert L.last_error()
    assert fc(W, L.shape_arr((360, 3, 3)), P_(src), n, P_(sky), P_(resp), P_(out), None) == -22       # ny < 4
    torch.cuda.synchronize()
    untouched = lambda: (bool((dst == -3.5).all()) and bool((sky == 0.25).all()) and bool((resp == 0.75).all()) and
                         bool((vals == 1.5).all()) and bool((src == 1.25).all()) and bool((out == -7.0).all()))
    assert untouched()
    # n = 0: nothing launched, whatever the pointers
    assert sb(W, shp, P_(dst), 0, 181, 0, None, None, None, 0, None) == 0 and sc(W, shp, P_(dst), 0, None, None, None, 1, None) == 0
    assert fb(W, shp, P_(src), 0, 181, 0, None, None, None, None) == 0 and fc(W, shp, P_(src), 0, None, None, None, None) == 0
    assert sb(W, shp, None, 90, 0, n, P_(sky), P_(resp), P_(vals), 0, None) == 0                 # an empty window
    torch.cuda.synchronize()
    assert untouched()
    # and the same arguments made valid do their work, on an explicit stream
    side = torch.cuda.Stream(device=dev)
    st = C.c_void_p(side.cuda_stream)
    assert sb(W, shp, P_(dst), 0, 181, n, P_(sky), P_(resp), P_(vals), 0, st) == 0, L.last_error()
    side.synchronize()
    assert int((dst != -3.5).sum()) == 3 * 4 and bool((dst[3:] == -3.5).all())
    assert sc(W, shp, P_(dst), n, P_(sky), P_(resp), P_(vals), 1, st) == 0, L.last_error()
    side.synchronize()
    assert int((dst != -3.5).sum()) == 6 * 16
    assert fb(W, shp, P_(src), 0, 181, n, P_(sky), P_(resp), P_(out), st) == 0, L.last_error()
    side.synchronize()
    want = (1.25 + 0.75 * 1.25) + 0.75 * 1.25
    assert bool(((out - want).abs() <= 16 * SR.EPS * want).all())                                # a lerp of equal values, within rounding
    out.fill_(-7.0)
    assert fc(W, shp, P_(src), n, P_(sky), P_(resp), P_(out), st) == 0, L.last_error()
    side.synchronize()
    assert bool(((out - want).abs() <= 16 * SR.EPS * want).all())                                # the sixteen weights sum to 1 within rounding


def test_wrapper_refusals(pj, dev):
    shape, wcs = _geometries(pj)["box_80x40"]
    sky = to_dev(R.sphere_points(100, 0), dev)
    resp = torch.ones((100, 2), dtype=torch.float64, device=dev)
    vals = torch.ones(100, dtype=torch.float64, device=dev)
    out = torch.zeros((6, 40, 80), dtype=torch.float64, device=dev)
    m = pj.Enmap(torch.zeros((3, 40, 80), dtype=torch.float64, device=dev), wcs)
    tan = pj.Gnomonic(wcs.cdelt, wcs.crpix, wcs.crval)
    for fn, np_ in ((pj.scatter_pol, 3), (pj.scatter_pol_weights, 6)):
        o = out[:np_]
        for kw in ({}, {"order": 3}, {"order": 3, "prefiltered": True}):
            with pytest.raises(ValueError, match="Float64"):
                fn(vals.float(), sky, resp, shape, wcs, **kw)
            with pytest.raises(ValueError, match="Float64"):
                fn(vals, sky.float(), resp, shape, wcs, **kw)
            with pytest.raises(ValueError, match="Float64"):
                fn(vals, sky, resp.float(), shape, wcs, **kw)
            with pytest.raises(ValueError, match="Float64"):
                fn(vals, sky, resp, shape, wcs, out=o.float(), **kw)
            with pytest.raises(ValueError, match="CAR only"):
                fn(vals, sky, resp, shape, tan, **kw)
            with pytest.raises(ValueError):
                fn(vals[:99].contiguous(), sky, resp, shape, wcs, out=o, **kw)
            with pytest.raises(ValueError):
                fn(torch.ones((3, 100), dtype=torch.float64, device=dev), sky, resp, shape, wcs, out=o, **kw)      # one value per point
            with pytest.raises(ValueError):
                fn(vals, sky, resp[:99].contiguous(), shape, wcs, out=o, **kw)
            with pytest.raises(ValueError):
                fn(vals, sky, resp.reshape(2, 100), shape, wcs, out=o, **kw)
            with pytest.raises(ValueError):
                fn(vals, sky, resp, shape, wcs, out=out[:9 - np_], **kw)                                        # the other mode's planes
            with pytest.raises(ValueError, match="overlaps"):
                fn(vals, sky, o.view(-1)[1000:1200].view(100, 2), shape, wcs, out=o, **kw)                     # resp overlaps out
            with pytest.raises(ValueError, match="overlaps"):
                fn(o.view(-1)[:100], sky, resp, shape, wcs, out=o, **kw)
        with pytest.raises(ValueError, match="order=1 only"):
            fn(vals, sky, resp, shape, wcs, order=3, out=o, src_rows=(0, 40), full_shape=shape)
        with pytest.raises(ValueError, match="order=3"):
            fn(vals, sky, resp, shape, wcs, out=o, prefiltered=True)
        with pytest.raises(ValueError, match="4 x 4"):
            fn(vals, sky, resp, (80, 3), wcs, order=3)
        with pytest.raises(ValueError):
            fn(vals, sky, resp, shape, wcs, out=o, src_rows=(30, 20), full_shape=shape)
    for kw in ({}, {"order": 3}, {"order": 3, "prefiltered": True}):
        with pytest.raises(ValueError, match="three components"):
            pj.sample_pol(pj.Enmap(out[:2], wcs), sky, resp, **kw)
        with pytest.raises(ValueError, match="three components"):
            pj.sample_pol(pj.Enmap(out[0], wcs), sky, resp, **kw)
        with pytest.raises(ValueError, match="Float"):
            pj.sample_pol(pj.Enmap(m.data.float(), wcs), sky, resp, **kw)
        with pytest.raises(ValueError, match="Float64"):
            pj.sample_pol(m, sky, resp.float(), **kw)
        with pytest.raises(ValueError, match="Float64"):
            pj.sample_pol(m, sky.float(), resp, **kw)
        with pytest.raises(ValueError):
            pj.sample_pol(m, sky, resp[:99].contiguous(), **kw)
        with pytest.raises(ValueError):
            pj.sample_pol(pj.Enmap(m.data, tan), sky, resp, **kw)
    with pytest.raises(ValueError, match="order=1 only"):
        pj.sample_pol(m, sky, resp, order=3, src_rows=(0, 40), full_shape=shape)
    with pytest.raises(ValueError, match="order=3"):
        pj.sample_pol(m, sky, resp, prefiltered=True)
    with pytest.raises(ValueError):
        pj.sample_pol(m, sky, resp, src_rows=(0, 39), full_shape=shape)                                        # the data is not that strip
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(m.data.abs().max()) == 0.0
    assert pj.scatter_pol(vals, sky, resp, shape, wcs, out=pj.Enmap(out[:3], wcs)).data.data_ptr() == out.data_ptr()
    assert pj.scatter_pol_weights(vals, sky, resp, shape, wcs, out=out).data.data_ptr() == out.data_ptr()
