"""The fused normal operator on the device: pj.normal_pol and pxl_normal_car_pol_bilinear_f64.

The contract is the composition scatter_pol(w * sample_pol(x), out=y): the same multiset of terms, bit for bit, the order of the
atomic adds into one pixel unspecified.  So every check has the form of tests/test_gpu_pol.py's transpose checks: the result is
held to k * 2^-52 * S per pixel (scatter_ref's derivation) against the numpy yardstick tests/normal_ref.py AND against the
device's own composition; a pixel that takes at most one non-zero term must have the same BITS; a pixel that takes nothing keeps
its bits.  Two device calls are never asserted bit-equal beyond that.  Each check prints its worst error / bound."""
import ctypes as C

import numpy as np
import pytest

import normal_ref as NR
import pol_ref as P
import scatter_ref as R
import tap_ref

torch = pytest.importorskip("torch")
import gpu_support
from gpu_support import dev, edge_points, held_inf, to_dev
pytestmark = pytest.mark.gpu

CHUNK = 256                      # the points one block takes per trip: blockDim.x (256) times PXL_NUNR = 1
LD = np.longdouble


def _geometries(pj):
    return tap_ref.geometries(pj, ("cc_360x181", "box_80x40", "cc_1024x513", "box_2x2", "box_5x7"))


def _check(pj, O, dev, shape, wcs, x, sky, resp, w, what, seed=3):
    """One accumulating call into a random map against the yardstick and the device's composition.  The composition's values are
    the device's own forward bits times w, multiplied on the host.  Returns (ref, k, S, got, out0)."""
    out0 = gpu_support.out0(3, shape[1], shape[0], seed)
    dsky, dresp = to_dev(sky, dev).reshape(-1, 2), to_dev(resp, dev).reshape(-1, 2)
    em = pj.Enmap(to_dev(x, dev), wcs)
    fwd = pj.sample_pol(em, dsky, dresp).cpu().numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        vals = np.asarray(w, dtype=np.float64) * fwd
        ref, k, S = NR.normal(O, wcs, shape, x, sky, resp, w, out=out0)
    comp = pj.scatter_pol(to_dev(vals, dev), dsky, dresp, shape, wcs, out=to_dev(out0, dev)).data.cpu().numpy()
    dst = to_dev(out0, dev)
    res = pj.normal_pol(em, to_dev(w, dev), dsky, dresp, out=dst)
    assert isinstance(res, pj.Enmap) and res.data.data_ptr() == dst.data_ptr()
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    held_inf(got, ref, k, S, what + " against the yardstick")
    held_inf(got, comp, k, S, what + " against the composition")
    with np.errstate(invalid="ignore", over="ignore"):
        single = P.nonzero_terms(O, wcs, shape, sky, vals, resp) <= 1
    for other, name in ((ref, "the yardstick"), (comp, "the composition")):
        nan = np.isnan(other[single])
        assert np.array_equal(got[single].view(np.int64)[~nan], other[single].view(np.int64)[~nan]), \
            "%s: a pixel with at most one non-zero term differs in bits from %s" % (what, name)
    idle = k == 1
    assert np.array_equal(got[idle].view(np.int64), out0[idle].view(np.int64)), what + ": a pixel that receives nothing changed"
    return ref, k, S, got, out0, int(single.sum()), int(idle.sum())


def _inputs(shape, n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(3, shape[1], shape[0])), rng.normal(size=(n, 2)), 10.0 ** rng.uniform(-1, 1, n)


# ---- 1. against the composition and the yardstick ----------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["cc_360x181", "box_80x40", "box_2x2"])
def test_against_the_composition_and_the_yardstick(pj, O, dev, geom):
    shape, wcs = _geometries(pj)[geom]
    n = 20011                                                        # 79 blocks, the last partial
    sky = edge_points(O, wcs, shape, n, 21, True)
    x, resp, w = _inputs(shape, n, 22)
    resp[200] = [0.0, 1.5]; w[201] = 0.0                             # zero terms still add, and change nothing
    ref, k, S, got, out0, single, idle = _check(pj, O, dev, shape, wcs, x, sky, resp, w, geom)
    print("%s: %d pixels with at most one non-zero term, %d untouched, max k = %d" % (geom, single, idle, int(k.max())))
    assert np.isfinite(got).all() and (k > 1).any()
    if geom == "cc_360x181":
        assert idle > 0 and single > idle, "pixels left alone and pixels with one term exist on the sparse map"
    # out=None is a map of zeros
    fresh = pj.normal_pol(pj.Enmap(to_dev(x, dev), wcs), to_dev(w, dev), to_dev(sky, dev), to_dev(resp, dev))
    assert isinstance(fresh, pj.Enmap) and tuple(fresh.data.shape) == (3, shape[1], shape[0])
    r0, k0, S0 = NR.normal(O, wcs, shape, x, sky, resp, w)
    held_inf(fresh.data.cpu().numpy(), r0, k0, S0, geom + ", fresh map")


# ---- 2. batch sizes -------------------------------------------------------------------------------------------------------------------
def test_batch_sizes(pj, O, dev):
    shape, wcs = _geometries(pj)["cc_360x181"]
    for n in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1):
        sky = R.sphere_points(n, n + 1).reshape(-1, 2)
        x, resp, w = _inputs(shape, n, 30 + n)
        ref, k, S, got, out0, _s, _i = _check(pj, O, dev, shape, wcs, x, sky, resp, w, "n = %d" % n, seed=n)
        if n == 0:
            assert np.array_equal(got.view(np.int64), out0.view(np.int64))
        else:
            assert int((k > 1).sum()) >= 3 and int((k > 1).sum()) <= 12 * n


# ---- 3. contention --------------------------------------------------------------------------------------------------------------------
def test_contention_in_one_cell(pj, O, dev):
    shape, wcs = _geometries(pj)["cc_360x181"]
    n = 10 ** 5
    rng = np.random.default_rng(31)
    pix = np.stack([rng.uniform(100.001, 100.999, n), rng.uniform(50.001, 50.999, n)], axis=1)
    sky = O.pix2sky(wcs, pix, O.WRAP_NONE)
    x, resp, w = _inputs(shape, n, 32)
    ref, k, S, got, out0, _s, _i = _check(pj, O, dev, shape, wcs, x, sky, resp, w, "one cell")
    assert int((k > 1).sum()) == 12 and int(k.max()) == n + 1


# ---- 4. special values ----------------------------------------------------------------------------------------------------------------
def test_special_values_follow_the_composition(pj, O, dev):
    """A NaN and an Inf pixel in x and a NaN weight: the NaN (and infinite) pixels of y are exactly the composition's and the
    yardstick's -- the four taps, in all three planes, of every point that reads one of them, zero-weight taps included -- and
    every other pixel is held as in test 1."""
    shape, wcs = _geometries(pj)["box_80x40"]
    n = 20011
    sky = edge_points(O, wcs, shape, n, 41, True)
    centre = O.pix2sky(wcs, np.array([[30.0, 20.0], [61.0, 11.0], [12.0, 33.0]]), O.WRAP_NONE)
    sky[5000:5003] = centre                                          # pixel centres: zero-weight taps read the special pixels too
    x, resp, w = _inputs(shape, n, 42)
    x[1, 19, 29] = np.nan                                            # plane Q, pixel (30, 20)
    x[0, 10, 60] = np.inf                                            # plane I, pixel (61, 11)
    w[5002] = np.nan
    ref, k, S, got, out0, _s, _i = _check(pj, O, dev, shape, wcs, x, sky, resp, w, "special values")
    assert np.isnan(got).any() and np.isinf(got).any()
    idx, _w = R.taps(O, wcs, shape, sky)
    poisoned = (idx == 19 * 80 + 29).any(axis=1) | (idx == 10 * 80 + 60).any(axis=1)          # reads the NaN or the Inf pixel of x
    poisoned[5002] = True
    want = np.zeros(shape[0] * shape[1], bool)
    want[idx[poisoned][idx[poisoned] >= 0]] = True
    for c in range(3):
        assert np.array_equal(~np.isfinite(got[c]).ravel(), want), "plane %d: the non-finite pixels are not the taps of the points that read a special value" % c
    bad = want
    print("special values: %d points read a special value, %d pixels not finite" % (int(poisoned.sum()), int(bad.sum())))


# ---- 5. symmetry and positivity -------------------------------------------------------------------------------------------------------
def test_symmetry_and_positivity(pj, O, dev):
    """|<y, A x> - <A y, x>| and |<x, A x> - sum_k w_k (P x)_k^2| on box_80x40 with 2 * 10^5 points, in long double, against bounds
    from the yardstick's terms.  In exact arithmetic both vanish.  The device's (A x)_p is a sum of k_p terms, each a product
    chain of at most 15 roundings from a tap of x (6 in the three nested lerps, 3 in the combination, 1 for w, 3 for the product
    weight, 1 for q v or u v, 1 for the term; a 16th allowed for the second-order terms), summed in an order that costs at most
    2 k_p 2^-53 S_p between any two orders.  With Sabs_p = sum |term| formed WITHOUT cancellation (the yardstick on |x| and |resp|:
    every |term| of the real call is at most the corresponding one there), |(A x)_p - exact| <= 2^-53 (16 + 2 k_p) Sabs_p, so
        |<y, A x> - <A y, x>| <= 2^-53 sum_p (|y_p| (16 + 2 k_p) Sabs_p(x) + |x_p| (16 + 2 k_p) Sabs_p(y)).
    sum_k w_k (P x)_k^2 from the yardstick's forward carries at most 9 roundings per sample, twice, against sum_k w_k D_k^2 with
    D = P_abs |x|: 18 * 2^-53 of it."""
    shape, wcs = _geometries(pj)["box_80x40"]
    n = 2 * 10 ** 5
    sky = R.box_points(O, wcs, shape, n, 51)
    rng = np.random.default_rng(52)
    x, y = rng.normal(size=(3,) + (shape[1], shape[0])), rng.normal(size=(3,) + (shape[1], shape[0]))
    psi = rng.uniform(0, np.pi, n)
    resp = np.stack([np.cos(2 * psi), np.sin(2 * psi)], axis=1)
    w = 10.0 ** rng.uniform(-1, 1, n)
    dsky, dresp, dw = to_dev(sky, dev), to_dev(resp, dev), to_dev(w, dev)
    ax = pj.normal_pol(pj.Enmap(to_dev(x, dev), wcs), dw, dsky, dresp).data.cpu().numpy()
    ay = pj.normal_pol(pj.Enmap(to_dev(y, dev), wcs), dw, dsky, dresp).data.cpu().numpy()
    _rx, k, Sx = NR.normal(O, wcs, shape, np.abs(x), sky, np.abs(resp), w)
    _ry, _k, Sy = NR.normal(O, wcs, shape, np.abs(y), sky, np.abs(resp), w)
    c = (16 + 2 * k).astype(LD)
    bound = float(2.0 ** -53 * (np.sum(np.abs(y).astype(LD) * c * Sx.astype(LD)) + np.sum(np.abs(x).astype(LD) * c * Sy.astype(LD))))
    yax, ayx = np.sum(y.astype(LD) * ax.astype(LD)), np.sum(ay.astype(LD) * x.astype(LD))
    gap = float(abs(yax - ayx))
    print("symmetry: <y, A x> = %.6g, |<y, A x> - <A y, x>| = %.3g, bound %.3g" % (float(yax), gap, bound))
    assert 0 < bound < 1e-9 * float(np.sum(np.abs(y * ax))) and gap <= bound
    xax = np.sum(x.astype(LD) * ax.astype(LD))
    px = P.sample(O, wcs, shape, x, sky, resp)
    want = np.sum(w.astype(LD) * px.astype(LD) * px.astype(LD))
    D = P.sample(O, wcs, shape, np.abs(x), sky, np.abs(resp))
    bound2 = float(2.0 ** -53 * (np.sum(np.abs(x).astype(LD) * c * Sx.astype(LD)) + 18 * np.sum(w.astype(LD) * D.astype(LD) ** 2)))
    print("positivity: <x, A x> = %.6g, sum w (P x)^2 = %.6g, gap %.3g, bound %.3g" % (float(xax), float(want), float(abs(xax - want)), bound2))
    assert float(xax) > 0 and float(abs(xax - want)) <= bound2 < 1e-9 * float(want)


# ---- 6. the matrix itself --------------------------------------------------------------------------------------------------------------
def test_unit_maps_reproduce_the_dense_matrix(pj, O, dev):
    """box_5x7: A applied to each of the 105 unit maps is a column of D^T W D, D = pol_ref.dense(...), entry by entry to
    2^-53 (16 + 2 k_i) (|D|^T W |D|)_ij (test 5's count; k_i the number of terms pixel i takes).

    The six planes of pj.scatter_pol_weights are sum_k w_k wt_kp r r^T, the interpolation weight to the FIRST power, while the
    pixel-diagonal block of A carries wt_kp^2: the planes are not that block but the sum of the blocks of row p over all column
    pixels p' (sum_p' wt_kp' = 1 when every tap of every point is on the map, as here) -- the lumped blocks the preconditioner
    inverts.  That identity is what is checked, to the same bar summed over the row plus the planes' own k 2^-52 S and the
    4 * 2^-53 by which the four rounded product weights of a point may miss 1."""
    c = NR.case(pj, O, "box_5x7")
    shape, wcs = c.shape, c.wcs
    nx, ny = shape
    npix = nx * ny
    dsky, dresp, dw = to_dev(c.sky, dev), to_dev(c.resp, dev), to_dev(c.w, dev)
    got = np.empty((3 * npix, 3 * npix))
    e = torch.zeros((3, ny, nx), dtype=torch.float64, device=dev)
    for j in range(3 * npix):
        e.view(-1)[j] = 1.0
        got[:, j] = pj.normal_pol(pj.Enmap(e, wcs), dw, dsky, dresp).data.view(-1).cpu().numpy()
        e.view(-1)[j] = 0.0
    D = P.dense(O, wcs, shape, c.sky, c.resp).astype(LD)
    want = D.T @ (c.w.astype(LD)[:, None] * D)
    wabs = np.abs(D).T @ (c.w.astype(LD)[:, None] * np.abs(D))
    k = NR.normal(O, wcs, shape, c.m0, c.sky, c.resp, c.w)[1].reshape(-1)
    bar = 2.0 ** -53 * (16 + 2 * k).astype(LD)[:, None] * wabs
    err = np.abs(got.astype(LD) - want)
    print("unit maps: worst error / bound = %.3g over %d entries, %d of them non-zero" % (float((err[bar > 0] / bar[bar > 0]).max()), err.size, int((want != 0).sum())))
    assert np.all(err <= bar) and (want != 0).sum() > 9 * npix
    assert np.array_equal(got == 0, want == 0), "an entry outside the 3 x 3 pixel neighbourhood is not zero"
    idx, _wt = R.taps(O, wcs, shape, c.sky)
    assert (idx >= 0).all(), "every tap of every point is on the map"
    w6 = pj.scatter_pol_weights(dw, dsky, dresp, shape, wcs).data.cpu().numpy().reshape(6, npix)
    plane = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    for a in range(3):
        for b in range(3):
            rows = got[a * npix:(a + 1) * npix, b * npix:(b + 1) * npix].astype(LD).sum(axis=1)
            rbar = bar[a * npix:(a + 1) * npix, b * npix:(b + 1) * npix].sum(axis=1) + 2.0 ** -52 * (k[:npix] + 4) * wabs[a * npix:(a + 1) * npix, b * npix:(b + 1) * npix].sum(axis=1)
            assert np.all(np.abs(rows - w6[plane[(min(a, b), max(a, b))]]) <= rbar), (a, b)


# ---- 7. raw ABI and the wrapper's refusals ---------------------------------------------------------------------------------------------
def test_einval_leaves_every_buffer_untouched(pj, dev):
    lib = pj.load_library()
    L = pj._lib
    shape, wcs = _geometries(pj)["cc_360x181"]
    wc = wcs.to_struct()
    n = 2000
    npl = 181 * 360
    y = torch.full((4, 181, 360), -3.5, dtype=torch.float64, device=dev)      # a plane to spare for the overlap cases
    x = torch.full((3, 181, 360), 1.25, dtype=torch.float64, device=dev)
    sky = torch.full((n, 2), 0.25, dtype=torch.float64, device=dev)            # on the map: a call that ran would add
    resp = torch.full((n, 2), 0.75, dtype=torch.float64, device=dev)
    w = torch.full((n,), 1.5, dtype=torch.float64, device=dev)
    P_ = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    W = C.byref(wc)
    shp = L.shape_arr((360, 181, 3))
    fn = lib.pxl_normal_car_pol_bilinear_f64
    for nc in (1, 2, 4, 6):
        assert fn(W, L.shape_arr((360, 181, nc)), P_(x), P_(y), n, P_(sky), P_(resp), P_(w), None) == -22 and "3 components" in L.last_error()
    bad_wcs = type(wc)()
    bad = [
        (None, shp, P_(x), P_(y), n, P_(sky), P_(resp), P_(w)), (C.byref(bad_wcs), shp, P_(x), P_(y), n, P_(sky), P_(resp), P_(w)),
        (W, None, P_(x), P_(y), n, P_(sky), P_(resp), P_(w)), (W, L.shape_arr((0, 181, 3)), P_(x), P_(y), n, P_(sky), P_(resp), P_(w)),
        (W, shp, P_(x), P_(y), -1, P_(sky), P_(resp), P_(w)),                                  # n < 0
        (W, shp, None, P_(y), n, P_(sky), P_(resp), P_(w)), (W, shp, P_(x), None, n, P_(sky), P_(resp), P_(w)),   # null with n > 0
        (W, shp, P_(x), P_(y), n, None, P_(resp), P_(w)), (W, shp, P_(x), P_(y), n, P_(sky), None, P_(w)),
        (W, shp, P_(x), P_(y), n, P_(sky), P_(resp), None),
        (W, shp, P_(x), P_(y), n - 1, P_(sky, 8), P_(resp), P_(w)),                            # a 2xN batch not 16-byte aligned
        (W, shp, P_(x), P_(y), n - 1, P_(sky), P_(resp, 8), P_(w)),
        (W, shp, P_(x), P_(y), 2 ** 60, P_(sky), P_(resp), P_(w)),                             # 16 n overflows
        (W, L.shape_arr((2 ** 31, 2 ** 31, 3)), P_(x), P_(y), n, P_(sky), P_(resp), P_(w)),     # 24 nx ny overflows
        (W, shp, P_(x), P_(x), n, P_(sky), P_(resp), P_(w)),                                   # y is x
        (W, shp, P_(y, 8 * npl), P_(y), n, P_(sky), P_(resp), P_(w)),                          # y overlaps x in part
        (W, shp, P_(x), P_(y), n, P_(y, 16 * 3000), P_(resp), P_(w)),                          # y overlaps the points
        (W, shp, P_(x), P_(y), n, P_(sky), P_(y, 16 * 3000), P_(w)),                           # y overlaps the responses
        (W, shp, P_(x), P_(y), n, P_(sky), P_(resp), P_(y, 8 * 1000)),                         # y overlaps the weights
    ]
    for a in bad:
        assert fn(*a, None) == -22, a
        assert L.last_error()
    torch.cuda.synchronize()
    untouched = lambda: (bool((y == -3.5).all()) and bool((x == 1.25).all()) and bool((sky == 0.25).all()) and
                         bool((resp == 0.75).all()) and bool((w == 1.5).all()))
    assert untouched()
    assert fn(W, shp, None, None, 0, None, None, None, None) == 0                              # n = 0: nothing launched
    assert fn(W, shp, P_(x), P_(y), n, P_(sky), P_(resp), P_(y, 8 * 3 * npl), None) == 0       # w just past y's three planes is clear of it
    torch.cuda.synchronize()
    assert int((y[:3] != -3.5).sum()) == 3 * 4 and bool((y[3] == -3.5).all()) and bool((x == 1.25).all())
    y.fill_(-3.5)
    # and the valid call does its work, on an explicit stream
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    assert fn(W, shp, P_(x), P_(y), n, P_(sky), P_(resp), P_(w), C.c_void_p(side.cuda_stream)) == 0, L.last_error()
    side.synchronize()
    assert int((y != -3.5).sum()) == 3 * 4
    d = (1.25 + 0.75 * 1.25) + 0.75 * 1.25                                                     # a lerp of equal values, within rounding
    total = float((y[0] + 3.5).sum())
    assert abs(total - n * 1.5 * d) <= 1e-12 * n * 1.5 * d


def test_wrapper_refusals(pj, dev):
    shape, wcs = _geometries(pj)["box_80x40"]
    sky = to_dev(R.sphere_points(100, 0), dev)
    resp = torch.ones((100, 2), dtype=torch.float64, device=dev)
    w = torch.ones(100, dtype=torch.float64, device=dev)
    out = torch.zeros((3, 40, 80), dtype=torch.float64, device=dev)
    m = pj.Enmap(torch.zeros((3, 40, 80), dtype=torch.float64, device=dev), wcs)
    tan = pj.Gnomonic(wcs.cdelt, wcs.crpix, wcs.crval)
    with pytest.raises(TypeError):
        pj.normal_pol(m.data, w, sky, resp)
    with pytest.raises(ValueError, match="CAR only"):
        pj.normal_pol(pj.Enmap(m.data, tan), w, sky, resp)
    with pytest.raises(ValueError, match="three components"):
        pj.normal_pol(pj.Enmap(m.data[:2], wcs), w, sky, resp)
    with pytest.raises(ValueError, match="three components"):
        pj.normal_pol(pj.Enmap(m.data[0], wcs), w, sky, resp)
    for args, kw in (((pj.Enmap(m.data.float(), wcs), w, sky, resp), {}), ((m, w.float(), sky, resp), {}), ((m, w, sky.float(), resp), {}),
                     ((m, w, sky, resp.float()), {}), ((m, w, sky, resp), {"out": out.float()})):
        with pytest.raises(ValueError, match="Float64"):
            pj.normal_pol(*args, **kw)
    with pytest.raises(ValueError):
        pj.normal_pol(m, w[:99].contiguous(), sky, resp)
    with pytest.raises(ValueError):
        pj.normal_pol(m, w, sky, resp[:99].contiguous())
    with pytest.raises(ValueError):
        pj.normal_pol(m, w, sky.reshape(2, 100), resp)
    with pytest.raises(ValueError):
        pj.normal_pol(m, w, sky, resp, out=torch.zeros((3, 40, 81), dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError):
        pj.normal_pol(m, w.cpu(), sky, resp)
    for kw in ({"out": m}, {"out": m.data}):
        with pytest.raises(ValueError, match="overlaps"):
            pj.normal_pol(m, w, sky, resp, **kw)
    with pytest.raises(ValueError, match="overlaps"):
        pj.normal_pol(m, out.view(-1)[:100], sky, resp, out=out)
    with pytest.raises(ValueError, match="overlaps"):
        pj.normal_pol(m, w, out.view(-1)[1000:1200].view(100, 2), resp, out=out)
    with pytest.raises(ValueError, match="overlaps"):
        pj.normal_pol(m, w, sky, out.view(-1)[1000:1200].view(100, 2), out=out)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(m.data.abs().max()) == 0.0
    assert pj.normal_pol(m, w, sky, resp, out=out).data.data_ptr() == out.data_ptr()
    assert pj.normal_pol(m, w, sky, resp, out=pj.Enmap(out, wcs)).data.data_ptr() == out.data_ptr()
