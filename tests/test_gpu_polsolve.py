"""The per-pixel IQU block solve on the device: pj.pol_block_solve, pj.pol_block_apply, pj.binned_map_pol and
the two pxl_pol_block_* entries.

The solve, its rcond plane and the block product are compared with the numpy yardstick tests/polsolve_ref.py as BIT patterns,
NaN by position: the arithmetic is defined operation by operation (include/pixell_hip.h).  The binned map is held end to end
to a constant sky within a per-pixel bound derived in the test's docstring, and to the composition of the calls it is made of.
Each check prints its worst error / bound."""
import ctypes as C
import functools

import numpy as np
import pytest

import polsolve_ref as Q
import scatter_ref as R
from conftest import DEG

torch = pytest.importorskip("torch")
from gpu_support import dev, same_bits, to_dev
pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
# one wave, one trip of a 256-thread block in both forms (256 pixels element-wise, 512 with two pixels per lane), the 360 x 181 map
NPIX = [1, 2, 255, 256, 257, 511, 512, 513, 65160]
LEVELS = [1e-3, 1e-6]
M0 = np.array([1.5, -0.25, 0.4])                     # the constant sky (I0, Q0, U0)


@functools.lru_cache(maxsize=None)
def _mixed(npix):
    return Q.mixed_blocks(npix)


def _map_shape(npix):
    return (181, 360) if npix == 65160 else (1, npix)


def _same_bits(got, want, what):
    """gpu_support.same_bits of the flattened values: the device's (.., ny, nx) maps against the yardstick's (.., npix)."""
    same_bits(np.reshape(got, -1), np.reshape(want, -1), what)


def _wcs(pj):
    return pj.fullsky_geometry(1.0 * DEG)[1]


def _offset_tensor(a, dev):
    """A contiguous device copy of `a` that starts 8 bytes past a 16-byte boundary."""
    buf = torch.empty(a.size + 1, dtype=torch.float64, device=dev)
    assert buf.data_ptr() % 16 == 0
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert t.data_ptr() % 16 == 8 and t.is_contiguous()
    return t


# ---- 1. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("npix", NPIX)
def test_bits(pj, dev, npix, level):
    """pj.pol_block_solve, its rcond plane and pj.pol_block_apply against the yardstick, bit for bit: random pointing-matrix
    blocks of 0-11 hits, every special block (zero, NaN, +-Inf, negative, -0.0), the diagonal ties, and solved blocks under every
    relabelling of I, Q, U, so that each of the six (first pivot, second-pivot swap) orders is compared on non-zero values from
    npix = 255 up.  An even npix on torch's
    256-byte aligned buffers takes two pixels per lane, an odd one the element-wise kernel."""
    w6, r3 = _mixed(npix)
    ny, nx = _map_shape(npix)
    wcs = _wcs(pj)
    want, want_rc, info = Q.solve(w6, r3, level)
    wts = pj.Enmap(to_dev(w6.reshape(6, ny, nx), dev), wcs)
    rhs = pj.Enmap(to_dev(r3.reshape(3, ny, nx), dev), wcs)
    got, rc = pj.pol_block_solve(rhs, wts, rcond_min=level, return_rcond=True)
    assert isinstance(got, pj.Enmap) and isinstance(rc, pj.Enmap)
    assert tuple(got.data.shape) == (3, ny, nx) and tuple(rc.data.shape) == (ny, nx)
    what = "npix %d, rcond_min %g" % (npix, level)
    _same_bits(got.data.cpu().numpy(), want, "solve, " + what)
    _same_bits(rc.data.cpu().numpy(), want_rc, "rcond, " + what)
    _same_bits(rhs.data.cpu().numpy(), r3, "the right-hand side of an out-of-place call, " + what)
    if npix >= 255:
        assert info["ok"].sum() > npix // 4 and (~info["ok"]).sum() > 36, "solved and masked blocks both present"
        for i1 in (0, 1, 2):                             # every pivot order is compared on blocks that are solved, with non-zero bits
            for swap in (False, True):
                assert (info["ok"] & (info["i1"] == i1) & (info["swap"] == swap) & (want != 0).all(axis=0)).sum() >= 5, (i1, swap)
    y = pj.pol_block_apply(rhs, wts)
    _same_bits(y.data.cpu().numpy(), Q.apply(w6, r3), "apply, " + what)


@pytest.mark.parametrize("npix", [512, 65160])
def test_bits_eight_bytes_past_a_16_byte_boundary(pj, dev, npix):
    """An even npix whose buffers do not start on a 16-byte boundary: the element-wise kernel, the same bits."""
    w6, r3 = _mixed(npix)
    ny, nx = _map_shape(npix)
    wcs = _wcs(pj)
    wts = pj.Enmap(_offset_tensor(w6.reshape(6, ny, nx), dev), wcs)
    rhs = pj.Enmap(_offset_tensor(r3.reshape(3, ny, nx), dev), wcs)
    out = pj.Enmap(_offset_tensor(np.full((3, ny, nx), -7.0), dev), wcs)
    for level in LEVELS:
        want, want_rc, _info = Q.solve(w6, r3, level)
        got, rc = pj.pol_block_solve(rhs, wts, rcond_min=level, out=out, return_rcond=True)
        assert got.data.data_ptr() == out.data.data_ptr()
        _same_bits(got.data.cpu().numpy(), want, "offset solve, npix %d" % npix)
        _same_bits(rc.data.cpu().numpy(), want_rc, "offset rcond, npix %d" % npix)
    y = pj.pol_block_apply(rhs, wts, out=out)
    _same_bits(y.data.cpu().numpy(), Q.apply(w6, r3), "offset apply, npix %d" % npix)
    # only the right-hand side off the boundary, and in place
    wts2 = pj.Enmap(to_dev(w6.reshape(6, ny, nx), dev), wcs)
    got = pj.pol_block_solve(rhs, wts2, rcond_min=1e-3, out=rhs)
    _same_bits(got.data.cpu().numpy(), Q.solve(w6, r3, 1e-3)[0], "offset in place, npix %d" % npix)


# ---- 2. in place, and without the rcond plane --------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", [257, 512, 65160])
def test_in_place_and_without_rcond(pj, dev, npix):
    w6, r3 = _mixed(npix)
    ny, nx = _map_shape(npix)
    wcs = _wcs(pj)
    wts = pj.Enmap(to_dev(w6.reshape(6, ny, nx), dev), wcs)
    for level in LEVELS:
        rhs = pj.Enmap(to_dev(r3.reshape(3, ny, nx), dev), wcs)
        ref, ref_rc = pj.pol_block_solve(rhs, wts, rcond_min=level, return_rcond=True)
        plain = pj.pol_block_solve(rhs, wts, rcond_min=level)
        assert isinstance(plain, pj.Enmap)
        _same_bits(plain.data.cpu().numpy(), ref.data.cpu().numpy(), "without rcond, npix %d" % npix)
        for with_rc in (True, False):
            r = pj.Enmap(to_dev(r3.reshape(3, ny, nx), dev), wcs)
            res = pj.pol_block_solve(r, wts, rcond_min=level, out=r, return_rcond=with_rc)
            m = res[0] if with_rc else res
            assert m.data.data_ptr() == r.data.data_ptr()
            _same_bits(m.data.cpu().numpy(), ref.data.cpu().numpy(), "in place, npix %d" % npix)
            if with_rc:
                _same_bits(res[1].data.cpu().numpy(), ref_rc.data.cpu().numpy(), "in place rcond, npix %d" % npix)
    x = pj.Enmap(to_dev(r3.reshape(3, ny, nx), dev), wcs)
    y = pj.pol_block_apply(x, wts, out=x)
    assert y.data.data_ptr() == x.data.data_ptr()
    _same_bits(y.data.cpu().numpy(), Q.apply(w6, r3), "apply in place, npix %d" % npix)
    _same_bits(wts.data.cpu().numpy(), w6, "the weights")


# ---- 3. npix = 0, the raw ABI's refusals, the wrappers' refusals -----------------------------------------------------------------
def test_einval_leaves_every_buffer_untouched(pj, dev):
    lib = pj.load_library()
    L = pj._lib
    n = 1000
    wts = torch.full((6 * n,), 2.5, dtype=torch.float64, device=dev)
    rhs = torch.full((3 * n,), 1.25, dtype=torch.float64, device=dev)
    out = torch.full((3 * n,), -7.0, dtype=torch.float64, device=dev)
    rc = torch.full((n,), -3.5, dtype=torch.float64, device=dev)
    P_ = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    solve, apply = lib.pxl_pol_block_solve_f64, lib.pxl_pol_block_apply_f64
    bad_solve = [
        (None, P_(rhs), P_(out), P_(rc), n, 1e-3), (P_(wts), None, P_(out), P_(rc), n, 1e-3),         # null pointers with npix > 0
        (P_(wts), P_(rhs), None, P_(rc), n, 1e-3), (P_(wts), P_(rhs), None, None, n, 1e-3),
        (P_(wts), P_(rhs), P_(out), P_(rc), -1, 1e-3),                                               # npix < 0
        (P_(wts), P_(rhs), P_(out), P_(rc), n, float("nan")), (P_(wts), P_(rhs), P_(out), P_(rc), n, float("inf")),
        (P_(wts), P_(rhs), P_(out), P_(rc), n, 0.0), (P_(wts), P_(rhs), P_(out), P_(rc), n, -1e-3),  # rcond_min outside (0, 1]
        (P_(wts), P_(rhs), P_(out), P_(rc), n, 1.0000001), (P_(wts), P_(rhs), P_(out), None, n, 2.0),
        (P_(wts), P_(rhs), P_(wts, 8 * 3 * n), P_(rc), n, 1e-3),                                     # out inside the weights
        (P_(wts), P_(rhs), P_(wts, 8 * 5 * n), None, n, 1e-3),                                       # out across the weights' end
        (P_(out, 8 * 100), P_(rhs), P_(out), P_(rc), n // 4, 1e-3),                                    # the weights' start inside out
        (P_(wts), P_(rhs), P_(out), P_(out, 8 * 2 * n), n, 1e-3),                                    # rcond inside out
        (P_(wts), P_(rhs), P_(rc), P_(rc), n // 3, 1e-3),                                            # rcond is out
        (P_(wts), P_(rhs), P_(rhs, 8), P_(rc), n - 1, 1e-3),                                         # out overlaps rhs, not exactly
        (P_(wts), P_(rhs, 8 * n), P_(rhs), P_(rc), n // 2, 1e-3),
        (P_(wts), P_(rhs), P_(out), P_(wts, 8 * 5 * n), n, 1e-3),                                    # rcond inside the weights
        (P_(wts), P_(rhs), P_(out), P_(rhs, 8 * n), n, 1e-3),                                        # rcond inside rhs
        (P_(wts), P_(rhs), P_(rhs), P_(rhs, 8 * 2 * n), n, 1e-3),                                    # in place, rcond inside rhs
        (P_(wts, 4), P_(rhs), P_(out), P_(rc), n - 1, 1e-3), (P_(wts), P_(rhs), P_(out, 4), P_(rc), n - 1, 1e-3),   # not 8-byte aligned
    ]
    for a in bad_solve:
        assert solve(*a, None) == -22, a
        assert L.last_error()
    bad_apply = [
        (None, P_(rhs), P_(out), n), (P_(wts), None, P_(out), n), (P_(wts), P_(rhs), None, n), (P_(wts), P_(rhs), P_(out), -1),
        (P_(wts), P_(rhs), P_(wts, 8 * 3 * n), n), (P_(wts), P_(rhs), P_(wts, 8 * 5 * n), n), (P_(out, 8 * 100), P_(rhs), P_(out), n // 4),
        (P_(wts), P_(rhs), P_(rhs, 8), n - 1), (P_(wts), P_(rhs, 8 * n), P_(rhs), n // 2), (P_(wts), P_(rhs, 4), P_(out), n - 1),
    ]
    for a in bad_apply:
        assert apply(*a, None) == -22, a
        assert L.last_error()
    torch.cuda.synchronize()
    untouched = lambda: (bool((wts == 2.5).all()) and bool((rhs == 1.25).all()) and bool((out == -7.0).all()) and bool((rc == -3.5).all()))
    assert untouched()
    # npix = 0: nothing launched, whatever the pointers
    assert solve(None, None, None, None, 0, 1e-3, None) == 0 and solve(P_(wts), P_(rhs), P_(out), P_(rc), 0, 1.0, None) == 0
    assert apply(None, None, None, 0, None) == 0 and apply(P_(wts), P_(rhs), P_(out), 0, None) == 0
    assert solve(None, None, None, None, 0, 0.0, None) == -22                                         # a bad rcond_min is refused at any size
    torch.cuda.synchronize()
    assert untouched()
    # and the same arguments made valid do their work, on an explicit stream: A = 2.5 * ones is singular, the identity is not
    side = torch.cuda.Stream(device=dev)
    st = C.c_void_p(side.cuda_stream)
    assert solve(P_(wts), P_(rhs), P_(out), P_(rc), n, 1e-3, st) == 0, L.last_error()
    side.synchronize()
    assert bool((out == 0).all()) and bool((rc == 0).all())
    wts.view(6, n)[1:3] = 0.0; wts.view(6, n)[4] = 0.0
    torch.cuda.synchronize()
    assert solve(P_(wts), P_(rhs), P_(out), None, n, 1.0, st) == 0, L.last_error()                     # rcond_min = 1 is allowed
    side.synchronize()
    assert bool((out == 0.5).all()) and bool((rc == 0).all())
    assert apply(P_(wts), P_(out), P_(out), n, st) == 0, L.last_error()                               # in place
    side.synchronize()
    assert bool((out == 1.25).all())


def test_wrapper_refusals(pj, dev):
    shape, wcs = pj.geometry([[20 * DEG, -20 * DEG], [-10 * DEG, 10 * DEG]], 0.5 * DEG)
    assert shape == (80, 40)
    tan = pj.Gnomonic(wcs.cdelt, wcs.crpix, wcs.crval)
    wd = torch.full((6, 40, 80), 2.5, dtype=torch.float64, device=dev)
    rd = torch.full((3, 40, 80), 1.25, dtype=torch.float64, device=dev)
    od = torch.full((3, 40, 80), -7.0, dtype=torch.float64, device=dev)
    w, r, o = pj.Enmap(wd, wcs), pj.Enmap(rd, wcs), pj.Enmap(od, wcs)
    E = pj.Enmap
    for fn in (pj.pol_block_solve, pj.pol_block_apply):
        with pytest.raises(TypeError):
            fn(rd, w)                                                              # not an Enmap
        with pytest.raises(TypeError):
            fn(r, wd)
        with pytest.raises(ValueError, match="3 planes"):
            fn(E(rd[:2], wcs), w)
        with pytest.raises(ValueError, match="3 planes"):
            fn(E(rd[0], wcs), w)
        with pytest.raises(ValueError, match="6 planes"):
            fn(r, E(wd[:5], wcs))
        with pytest.raises(ValueError, match="6 planes"):
            fn(r, E(wd[:3], wcs))
        with pytest.raises(ValueError):
            fn(r, E(wd[:, :39].contiguous(), wcs))                                 # another map size
        with pytest.raises(ValueError):
            fn(E(rd[:, :, :79].contiguous(), wcs), w)
        with pytest.raises(ValueError, match="Float64"):
            fn(E(rd.float(), wcs), w)
        with pytest.raises(ValueError, match="Float64"):
            fn(r, E(wd.float(), wcs))
        with pytest.raises(ValueError, match="Float64"):
            fn(r, w, out=E(od.float(), wcs))
        with pytest.raises(RuntimeError, match="GPU"):
            fn(E(rd.cpu(), wcs), w)
        with pytest.raises(RuntimeError, match="GPU"):
            fn(r, E(wd.cpu(), wcs))
        with pytest.raises(RuntimeError, match="GPU"):
            fn(r, w, out=E(od.cpu(), wcs))
        with pytest.raises(ValueError, match="contiguous"):
            fn(E(rd[:, :, ::2], wcs), E(wd[:, :, ::2], wcs))
        with pytest.raises(ValueError, match="contiguous"):
            fn(r, E(wd.permute(0, 2, 1).contiguous().permute(0, 2, 1), wcs))
        with pytest.raises(ValueError, match="contiguous"):
            fn(r, w, out=E(od.permute(0, 2, 1).contiguous().permute(0, 2, 1), wcs))
        with pytest.raises(ValueError, match="CAR only"):
            fn(E(rd, tan), w)
        with pytest.raises(ValueError, match="CAR only"):
            fn(r, E(wd, tan))
        with pytest.raises(ValueError):
            fn(r, w, out=E(od[:2], wcs))
        with pytest.raises(ValueError, match="overlaps"):
            fn(r, w, out=E(wd[:3], wcs))
        with pytest.raises(ValueError, match="overlaps"):
            fn(r, w, out=E(wd[3:], wcs))
        with pytest.raises(ValueError, match="overlaps"):
            fn(E(wd[1:4], wcs), E(torch.ones_like(wd), wcs), out=E(wd[2:5], wcs))  # out overlaps the input, not exactly
    for bad in (0.0, -1e-3, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rcond_min"):
            pj.pol_block_solve(r, w, rcond_min=bad)
        with pytest.raises(ValueError, match="rcond_min"):
            pj.pol_block_solve(r, w, rcond_min=bad, out=r, return_rcond=True)
    # binned_map_pol: its own checks, then scatter_pol's
    sky = to_dev(R.sphere_points(100, 0), dev)
    resp = torch.ones((100, 2), dtype=torch.float64, device=dev)
    d = torch.ones(100, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="Float64"):
        pj.binned_map_pol(d.float(), d, sky, resp, shape, wcs)
    with pytest.raises(ValueError, match="Float64"):
        pj.binned_map_pol(d, d.float(), sky, resp, shape, wcs)
    with pytest.raises(ValueError):
        pj.binned_map_pol(d, d[:99].contiguous(), sky, resp, shape, wcs)
    with pytest.raises(RuntimeError, match="GPU"):
        pj.binned_map_pol(d.cpu(), d, sky, resp, shape, wcs)
    with pytest.raises(ValueError, match="rcond_min"):
        pj.binned_map_pol(d, d, sky, resp, shape, wcs, rcond_min=0.0)
    with pytest.raises(ValueError, match="CAR only"):
        pj.binned_map_pol(d, d, sky, resp, shape, tan)
    with pytest.raises(ValueError, match="Float64"):
        pj.binned_map_pol(d, d, sky, resp.float(), shape, wcs)
    with pytest.raises(ValueError):
        pj.binned_map_pol(d, d, sky[:99].contiguous(), resp, shape, wcs)
    with pytest.raises(TypeError):
        pj.binned_map_pol(d, d, sky, resp, shape, wcs, order=3)                    # order 1 only: there is no such argument
    torch.cuda.synchronize()
    assert bool((wd == 2.5).all()) and bool((rd == 1.25).all()) and bool((od == -7.0).all())
    # an empty map is no error, and the accepted forms of `out`
    e = pj.pol_block_solve(E(rd[:, :0], wcs), E(wd[:, :0], wcs), return_rcond=True)
    assert tuple(e[0].data.shape) == (3, 0, 80) and tuple(e[1].data.shape) == (0, 80)
    assert pj.pol_block_solve(r, w, out=od).data.data_ptr() == od.data_ptr()       # a bare tensor
    assert pj.pol_block_solve(r, w, out=o) is o
    torch.cuda.synchronize()
    assert bool((od == 0).all())                                                   # 2.5 * ones is singular


# ---- 4. the binned map, end to end -------------------------------------------------------------------------------------------------
def _constant_sky_case(pj, O, dev, geom):
    """Inputs and host-side bookkeeping of one geometry, computed once: the points, responses, weights and noise-free samples
    of the constant sky M0, and per pixel the adder count k and the number of non-zero terms."""
    if geom == "cc_360x181":
        shape, wcs = pj.fullsky_geometry(1.0 * DEG)
        n = 10 ** 6
        dsky = torch.empty((n, 2), dtype=torch.float64, device=dev)
        pj.fill_sphere_points_(dsky, 7)
        sky = dsky.cpu().numpy()
    else:
        if geom == "box_80x40":
            shape, wcs = pj.geometry([[20 * DEG, -20 * DEG], [-10 * DEG, 10 * DEG]], 0.5 * DEG)
            n = 2 * 10 ** 5
        else:
            shape, wcs = pj.geometry([[2.5 * DEG, -2.5 * DEG], [-3.5 * DEG, 3.5 * DEG]], 1.0 * DEG)
            n = 2 * 10 ** 4
        sky = R.box_points(O, wcs, shape, n, 21)
        dsky = to_dev(sky, dev)
    assert shape == {"cc_360x181": (360, 181), "box_80x40": (80, 40), "box_5x7": (5, 7)}[geom]
    rng = np.random.default_rng(len(geom))
    psi = rng.uniform(0, np.pi, n)
    resp = np.stack([np.cos(2 * psi), np.sin(2 * psi)], axis=1)
    w = rng.uniform(0.5, 2.0, n)
    d = (M0[0] + resp[:, 0] * M0[1]) + resp[:, 1] * M0[2]
    # k: how many taps land on the pixel -- the term count scatter_ref.scatter, the yardstick of scatter_bilinear, returns for a
    # scatter of ones, here as a bincount over its taps.  The device's scatter_bilinear of ones gives the SUM of the taps' weights,
    # from which a count cannot be read; it is held to k below: nothing where k = 0, at most k elsewhere.
    idx, tw = R.taps(O, wcs, shape, sky)
    npix = shape[0] * shape[1]
    on = idx >= 0
    k = np.bincount(idx[on], minlength=npix).reshape(shape[1], shape[0])
    nz = np.bincount(idx[on & (tw != 0)], minlength=npix).reshape(shape[1], shape[0])
    ones = pj.scatter_bilinear(torch.ones(n, dtype=torch.float64, device=dev), dsky, shape, wcs).data.cpu().numpy()
    assert not ones[k == 0].any() and np.all(ones <= k * (1 + k * EPS)) and np.array_equal(ones > 0, nz > 0)
    return {"shape": shape, "wcs": wcs, "n": n, "dsky": dsky, "dresp": to_dev(resp, dev), "dw": to_dev(w, dev), "dd": to_dev(d, dev), "k": k, "nz": nz}


@pytest.fixture(scope="module")
def fullsky(pj, O, dev):
    return _constant_sky_case(pj, O, dev, "cc_360x181")


C1, K0 = 16.0, 50.0


def _constant_sky_check(pj, case, geom, min_solved):
    m, rc = pj.binned_map_pol(case["dd"], case["dw"], case["dsky"], case["dresp"], case["shape"], case["wcs"])
    assert isinstance(m, pj.Enmap) and isinstance(rc, pj.Enmap)
    nx, ny = case["shape"]
    assert tuple(m.data.shape) == (3, ny, nx) and tuple(rc.data.shape) == (ny, nx)
    m, rc = m.data.cpu().numpy(), rc.data.cpu().numpy()
    assert np.isfinite(m).all() and np.isfinite(rc).all() and np.all(rc >= 0) and np.all(rc <= 1)
    solved = rc >= 1e-3
    share = float(solved.mean())
    few = case["k"] < 3
    print("%s: %.2f %% of %d pixels solved; %.2f %% have at least three adders" % (geom, 100 * share, solved.size, 100 * float((~few).mean())))
    assert share >= min_solved
    assert not solved[few].any(), "a pixel with fewer than three adders was solved"
    masked = m[:, ~solved]
    assert np.array_equal(masked.view(np.int64), np.zeros(masked.shape, np.int64)), "an unsolved pixel is not +0.0 in every plane"
    gap = np.abs(m - M0[:, None, None]).max(axis=0)[solved]
    bound = C1 * (case["k"][solved] + K0) * EPS * np.abs(M0).sum() / rc[solved]
    print("%s: worst gap / bound = %.3g; worst gap * rc / (k * 2^-52) = %.3g" % (
        geom, float((gap / bound).max()), float((gap * rc[solved] / (case["k"][solved] * EPS)).max())))
    assert np.all(gap <= bound)
    return m, rc, solved


def test_constant_sky_full_sky(pj, fullsky):
    """pj.binned_map_pol of the noise-free samples d = (I0 + q Q0) + u U0 of a constant sky m0 = (1.5, -0.25, 0.4), random psi,
    w in [0.5, 2], 10^6 points uniform on the sphere into the 360 x 181 map: every solved pixel returns m0 within

        16 (k + 50) 2^-52 ||m0||_1 / rc,        k the pixel's adder count (taps that land on it), rc its rcond.

    Derivation (u = 2^-53).  Per pixel the planes are sums of k terms om w p p^T (weights) and om w p d (right-hand side) with
    p = (1, q, u), |q|, |u| <= 1, and om = fl(wy wx) the SAME number in both, so it counts as exact.  In exact arithmetic
    A m0 = r.  The computed planes leave the residual rho = r^ - A^ m0:
      - d carries |dd| <= u (2 |I0| + 3 |q Q0| + 2 |u U0|) <= 3u ||m0||_1, and a right-hand-side term three more roundings
        (w d, q v, om t) on |om w p_c d| <= om w ||m0||_1: 6u om w ||m0||_1 per term;
      - a weight term has at most three roundings (q w, q t1, om t): 3u om w per entry, 3u om w ||m0||_1 in a row of A^ m0;
      - the k adds of a plane, in any order, move it by at most k u sum|term|: 2 k u sum(om w) ||m0||_1 for the two sides.
    sum(om w) is the II plane, which is p1 (q^2, u^2 <= 1), so ||rho||_inf <= (9 + 2k) u p1 ||m0||_1.  With A = L D L^T,
    |l_ij| <= 1 under diagonal pivoting, ||L^-1||_inf <= 4 and ||L^-T||_inf <= 4, so ||A^-1||_inf <= 16 / min(p2, p3) =
    16 / (rc p1), and the exact solution of the computed system is within 16 (9 + 2k) u ||m0||_1 / rc = (16 k + 72) 2^-52
    ||m0||_1 / rc of m0.  The solve itself (polsolve_ref.C_LAPACK's derivation) adds kappa_inf * 30u ||x||_inf with
    kappa_inf <= 3 p1 * 16 / (rc p1): 720 * 2^-52 ||m0||_1 / rc.  Together (16 k + 792) 2^-52 ||m0||_1 / rc; k0 = 50 leaves
    8 * 2^-52 for the second-order terms.

    Not vacuous: at least 95 % of the pixels are solved (the pole rows' pixels are too small to be hit three times), no pixel
    with fewer than three adders is, and every unsolved pixel is +0.0 in all three planes."""
    _constant_sky_check(pj, fullsky, "cc_360x181", 0.95)


@pytest.mark.parametrize("geom", ["box_80x40", "box_5x7"])
def test_constant_sky_boxes(pj, O, dev, geom):
    """The same on the 80 x 40 box with 2 * 10^5 points and the 5 x 7 box with 2 * 10^4, spread over the box widened by 1.5
    pixels (edge taps dropped): every pixel is solved."""
    _constant_sky_check(pj, _constant_sky_case(pj, O, dev, geom), geom, 1.0)


def test_against_the_composition(pj, fullsky):
    """On the full-sky inputs the binned map against pj.pol_block_solve(pj.scatter_pol(w d), pj.scatter_pol_weights(w)) run
    separately.  A pixel that takes at most one non-zero term has the same planes in both runs, so the same bits in the map and
    in rcond.  Elsewhere two runs of a scatter differ by up to k 2^-52 S per plane (scatter_ref), S <= p1 for a weight plane and
    <= p1 ||m0||_1 for the right-hand side: ||dr||_inf + ||dA||_inf ||x||_inf <= k 2^-52 p1 (1 + 3) ||m0||_1, through
    ||A^-1||_inf <= 16 / (rc p1) that is 64 k 2^-52 ||m0||_1 / rc, and each solve adds its 720: (64 k + 1440) 2^-52 ||m0||_1 / rc
    on pixels solved in both, rc the smaller of the two."""
    c = fullsky
    m, rc = pj.binned_map_pol(c["dd"], c["dw"], c["dsky"], c["dresp"], c["shape"], c["wcs"])
    rhs = pj.scatter_pol(c["dw"] * c["dd"], c["dsky"], c["dresp"], c["shape"], c["wcs"])
    wts = pj.scatter_pol_weights(c["dw"], c["dsky"], c["dresp"], c["shape"], c["wcs"])
    m2, rc2 = pj.pol_block_solve(rhs, wts, return_rcond=True)
    m, rc, m2, rc2 = m.data.cpu().numpy(), rc.data.cpu().numpy(), m2.data.cpu().numpy(), rc2.data.cpu().numpy()
    single = c["nz"] <= 1
    assert single.sum() > 100
    assert np.array_equal(m[:, single].view(np.int64), m2[:, single].view(np.int64))
    assert np.array_equal(rc[single].view(np.int64), rc2[single].view(np.int64))
    s1, s2 = rc >= 1e-3, rc2 >= 1e-3
    assert np.array_equal(s1, s2), "%d pixels solved in one run only" % int((s1 != s2).sum())
    gap = np.abs(m - m2).max(axis=0)[s1]
    bound = (64.0 * c["k"][s1] + 1440.0) * EPS * np.abs(M0).sum() / np.minimum(rc, rc2)[s1]
    print("binned map against the composition: worst gap / bound = %.3g on %d solved pixels; %d pixels compared as bits" % (
        float((gap / bound).max()), int(s1.sum()), int(single.sum())))
    assert np.all(gap <= bound)
    assert np.array_equal(m[:, ~s1].view(np.int64), m2[:, ~s1].view(np.int64))


# ---- 5. singular scans -----------------------------------------------------------------------------------------------------------------
def test_singular_scans_are_masked(pj, O, dev, fullsky):
    """What the adjugate / determinant route gets wrong.  All points at one psi: every block is a multiple of one p p^T, so no
    pixel is solved at 1e-3 and rcond is finite and below 1e-12 everywhere.  One point only: rank 1 on its four pixels, none
    solved, the rest of the map the zero block."""
    c = fullsky
    nx, ny = c["shape"]
    resp = torch.empty_like(c["dresp"])
    resp[:, 0] = float(np.cos(2 * 0.3)); resp[:, 1] = float(np.sin(2 * 0.3))
    d = torch.full_like(c["dd"], float((M0[0] + np.cos(0.6) * M0[1]) + np.sin(0.6) * M0[2]))
    m, rc = pj.binned_map_pol(d, c["dw"], c["dsky"], resp, c["shape"], c["wcs"])
    m, rc = m.data.cpu().numpy(), rc.data.cpu().numpy()
    assert np.isfinite(rc).all() and np.all(rc >= 0) and np.all(rc < 1e-12), "one angle: worst rcond %g" % float(rc.max())
    assert np.array_equal(m.view(np.int64), np.zeros(m.shape, np.int64))
    print("one angle: largest rcond %.3g over %d pixels, %d of them hit" % (float(rc.max()), rc.size, int((c["k"] > 0).sum())))
    # one point in the middle of a cell
    sky1 = O.pix2sky(c["wcs"], np.array([[100.3, 50.6]]), O.WRAP_NONE)
    one = lambda v: torch.full((1,), float(v), dtype=torch.float64, device=dev)
    m, rc = pj.binned_map_pol(one(1.0), one(1.5), to_dev(sky1, dev), to_dev(np.array([[np.cos(1.0), np.sin(1.0)]]), dev), c["shape"], c["wcs"])
    wts = pj.scatter_pol_weights(one(1.5), to_dev(sky1, dev), to_dev(np.array([[np.cos(1.0), np.sin(1.0)]]), dev), c["shape"], c["wcs"]).data.cpu().numpy()
    hit = wts[0] != 0
    assert int(hit.sum()) == 4
    m, rc = m.data.cpu().numpy(), rc.data.cpu().numpy()
    assert np.isfinite(rc).all() and np.all(rc[hit] < 1e-12) and np.all(rc >= 0) and not rc[~hit].any()
    assert np.array_equal(m.view(np.int64), np.zeros(m.shape, np.int64))
    print("one point: rcond on its four pixels %s" % rc[hit])
