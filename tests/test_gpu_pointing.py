"""Detector pointing expansion on the device: pj.expand_pointing over pxl_pointing_expand_f64, and the two
map-makers that expand chunk by chunk, pj.binned_map_pol_nearest_tod and pj.cg_map_pol_tod.

Accuracy is against the long-double truth of tests/pointing_ref.py (the definition written out literally), never against the
code under test: the great-circle separation of (ra, dec) in units of 2^-52 rad and max(|dq|, |du|) in units of 2^-52 gamma / h.
THE BOUND is four times the worst value the Float64 numpy yardstick reaches against the same truth on the reference set below
(2 * 10^4 random unnormalised pairs and a polar set with h from 1e-12 to 1e-1), computed once here and shared by every case.
Each case's inputs are drawn like the reference set's (the small shapes hold a handful of samples: the yardstick's worst over
three samples would be no bound).  Measured on the MI355X when written: yardstick 2.50 and 3.26 on the reference set (bound 10.0 and 13.0), device 2.63 and 2.67 at worst over
the 60 cases."""
import numpy as np
import pytest

import nearest_ref as N
import pointing_ref as ref
import scatter_ref as R

torch = pytest.importorskip("torch")
from gpu_support import bits, dev, to_dev
pytestmark = pytest.mark.gpu

BLOCK_T = 256                    # the time samples one block takes per trip: PXL_PT_BLOCK, one per lane
GROUP_D = 8                      # the detectors a thread loops over with its boresight sample in registers: PXL_PT_GROUP
L = np.longdouble
OUT = ("ra", "dec", "q", "u")


def _device(pj, dev, qb, qd, gamma=None, **kw):
    sky, resp = pj.expand_pointing(to_dev(qb, dev), to_dev(qd, dev), None if gamma is None else to_dev(gamma, dev), **kw)
    sky, resp = sky.cpu().numpy(), resp.cpu().numpy()
    return {"ra": sky[:, 0], "dec": sky[:, 1], "q": resp[:, 0], "u": resp[:, 1]}


def _inputs(nd, nt, kind, seed):
    """(q_bore (T, 4), q_det (D, 4)).  random: unnormalised, norms 0.5 to 2.  polar: boresights within h of a pole, h from 1e-12
    to 1e-1, identity detectors scaled by 0.5 to 2.  identity: random boresights, detectors exactly (1, 0, 0, 0)."""
    rng = np.random.default_rng(seed)
    if kind == "polar":
        return ref.polar_quats(rng, nt), np.outer(rng.uniform(0.5, 2.0, nd), [1.0, 0.0, 0.0, 0.0])
    qd = np.tile([1.0, 0.0, 0.0, 0.0], (nd, 1)) if kind == "identity" else ref.random_quats(rng, nd)
    return ref.random_quats(rng, nt), qd


@pytest.fixture(scope="module")
def bound():
    """4 x the Float64 yardstick's worst (position, response) on the reference set."""
    rng = np.random.default_rng(2026)
    n = 20000
    qb = np.concatenate((ref.random_quats(rng, n), ref.polar_quats(rng, n // 4)))
    qd = ref.random_quats(rng, len(qb))
    qd[n:] = np.outer(rng.uniform(0.5, 2.0, n // 4), [1.0, 0.0, 0.0, 0.0])
    pos, resp = ref.worst(ref.expand_pairs(qb, qd), ref.expand_pairs(qb, qd, dtype=L))
    print("yardstick on the reference set: position %.2f x 2^-52 rad, response %.2f units; the device's bound is 4 x" % (pos, resp))
    return 4 * pos, 4 * resp


SHAPES = [(1, 1), (1, 2), (3, 257), (2, BLOCK_T - 1), (2, BLOCK_T), (2, BLOCK_T + 1), (GROUP_D - 1, 5), (GROUP_D, 5), (GROUP_D + 1, 5),
          (2 * GROUP_D + 3, 4 * BLOCK_T + 131)]          # the last: 19 x 1155 = 21945 samples, the last block partial both ways


@pytest.mark.parametrize("with_gamma", [False, True], ids=["gamma_null", "gamma"])
@pytest.mark.parametrize("kind", ["random", "polar", "identity"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_accuracy_against_long_double(pj, dev, bound, shape, kind, with_gamma):
    nd, nt = shape
    qb, qd = _inputs(nd, nt, kind, 1000 * nd + nt)
    gamma = np.random.default_rng(nd + nt).uniform(0.0, 1.0, nd) if with_gamma else None
    if with_gamma and nd > 2:
        gamma[1], gamma[2] = 0.0, 1.0
    got = _device(pj, dev, qb, qd, gamma)
    assert all(got[k].shape == (nd * nt,) for k in OUT)
    truth = ref.expand(qb, qd, gamma, dtype=L)
    g = None if gamma is None else np.repeat(gamma, nt)
    pos, resp = ref.worst(got, truth, g)
    print("%d x %d %s: position %.2f / %.2f, response %.2f / %.2f, worst ratio %.3f" % (nd, nt, kind, pos, bound[0], resp, bound[1],
                                                                                       max(pos / bound[0], resp / bound[1])))
    assert pos <= bound[0] and resp <= bound[1]
    assert np.all(got["ra"] > -np.pi) and np.all(got["ra"] <= np.pi) and np.all(np.abs(got["dec"]) <= np.pi / 2)
    # determinism: no atomics, so a second call and a call into given buffers give the same bits
    again = _device(pj, dev, qb, qd, gamma)
    sky, resp_buf = torch.full((nd * nt, 2), 7.0, dtype=torch.float64, device=dev), torch.full((nd * nt, 2), 7.0, dtype=torch.float64, device=dev)
    into = _device(pj, dev, qb, qd, gamma, out_sky=sky, out_resp=resp_buf)
    for k in OUT:
        assert np.array_equal(bits(got[k]), bits(again[k])) and np.array_equal(bits(got[k]), bits(into[k]))
    assert np.array_equal(bits(sky.cpu().numpy()[:, 0]), bits(got["ra"])) and np.array_equal(bits(resp_buf.cpu().numpy()[:, 1]), bits(got["u"]))


def test_out_buffers_are_returned(pj, dev):
    qb, qd = _inputs(3, 10, "random", 1)
    sky, resp = torch.empty((30, 2), dtype=torch.float64, device=dev), torch.empty((30, 2), dtype=torch.float64, device=dev)
    a, b = pj.expand_pointing(to_dev(qb, dev), to_dev(qd, dev), out_sky=sky, out_resp=resp)
    assert a is sky and b is resp
    a, b = pj.expand_pointing(to_dev(qb[:0], dev), to_dev(qd, dev))
    assert tuple(a.shape) == (0, 2) and tuple(b.shape) == (0, 2)


def test_special_values(pj, dev):
    """NaN, Inf and zero quaternions (and gammas) at chosen (d, t) make exactly those samples all-NaN, every other sample has the
    bits of a run without them; an exact-pole sample gives ra = +0.0 by bits."""
    nd, nt = GROUP_D + 3, BLOCK_T + 40
    qb, qd = _inputs(nd, nt, "random", 77)
    gamma = np.random.default_rng(78).uniform(0.1, 1.0, nd)
    clean = _device(pj, dev, qb, qd, gamma)
    qb2, qd2, g2 = qb.copy(), qd.copy(), gamma.copy()
    bad_t = {3: (0, np.nan), 64: (1, np.inf), 255: (2, -np.inf), 256: (3, np.nan), nt - 1: None}
    for t, how in bad_t.items():
        if how is None:
            qb2[t] = [0.0, -0.0, 0.0, 0.0]
        else:
            qb2[t, how[0]] = how[1]
    qd2[1, 2], qd2[GROUP_D] = np.inf, 0.0
    g2[4], g2[GROUP_D + 1] = np.nan, np.inf
    bad_d = {1, GROUP_D, 4, GROUP_D + 1}
    got = _device(pj, dev, qb2, qd2, g2)
    bad = np.zeros((nd, nt), bool)
    bad[sorted(bad_d), :] = True
    bad[:, sorted(bad_t)] = True
    bad = bad.reshape(-1)
    for k in OUT:
        assert np.isnan(got[k][bad]).all(), k
        assert np.array_equal(bits(got[k][~bad]), bits(clean[k][~bad])), k
    truth = ref.expand(qb2, qd2, g2, dtype=L)
    assert np.array_equal(np.isnan(truth["ra"].astype(np.float64)), bad)
    # the poles, exactly: every signed-zero form of a polar boresight (some give n_x = -0.0, where atan2 alone would answer pi), a
    # north pole with a position angle, and the branch cut n = (-2, -0.0, 0), where ra is +pi and never -pi
    qb = np.concatenate((ref.polar_sign_patterns(), [[np.cos(0.15), 0, 0, np.sin(0.15)], [1.0, 0.0, -1.0, -0.0]]))
    qd = np.array([[1.0, 0, 0, 0], [2.0, 0, 0, 0]])
    got = _device(pj, dev, qb, qd)
    truth = ref.expand(qb, qd, dtype=L)
    assert (np.signbit(truth["nx"].astype(np.float64)) & (truth["nx"] == 0)).any()
    nt = len(qb)
    for d in range(2):
        for t in range(nt - 1):
            k = d * nt + t
            assert bits(got["ra"][k]) == 0 and abs(got["dec"][k]) == np.pi / 2, (d, t, got["ra"][k], got["dec"][k])
            assert np.sign(got["dec"][k]) == np.sign(float(truth["dec"][k]))
            assert abs(got["q"][k] - float(truth["q"][k])) <= 4 * ref.EPS and abs(got["u"][k] - float(truth["u"][k])) <= 4 * ref.EPS
        assert got["ra"][d * nt + nt - 1] == np.pi


def test_the_convention_round_trip(pj, dev):
    """quat_from_radec -> expand_pointing with an identity detector gives back (ra, dec) and (cos 2 psi, sin 2 psi); a detector built
    as conj(q_b) (x) q_d looks where q_d says."""
    rng = np.random.default_rng(12)
    n = 5000
    ra, psi, dec = rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n), np.arcsin(rng.uniform(-1, 1, n))
    q = pj.quat_from_radec(torch.from_numpy(ra), torch.from_numpy(dec), torch.from_numpy(psi))
    sky, resp = pj.expand_pointing(q.to(dev), to_dev([[1.0, 0, 0, 0]], dev))
    sky, resp = sky.cpu().numpy(), resp.cpu().numpy()
    sep = ref.separation(sky[:, 0], sky[:, 1], {"ra": ra, "dec": dec}) * ref.EPS
    err = np.maximum(np.abs(resp[:, 0] - np.cos(2 * psi)), np.abs(resp[:, 1] - np.sin(2 * psi))) * np.cos(dec)
    print("round trip on the device: separation %.2e rad, response x h %.2e" % (sep.max(), err.max()))
    assert sep.max() <= 4e-15 and err.max() <= 2e-14
    qb, qd = q[:9], q[9:18]
    det = pj.quat_mul(pj.quat_conj(qb[4:5]), qd)                   # nine detectors as offsets from boresight sample 4
    sky, resp = pj.expand_pointing(qb.to(dev), det.to(dev))
    sky = sky.cpu().numpy().reshape(9, 9, 2)[:, 4]
    assert (ref.separation(sky[:, 0], sky[:, 1], {"ra": ra[9:18], "dec": dec[9:18]}) * ref.EPS).max() <= 8e-15


# ---- end to end: time-ordered data and quaternion pointing to a map ----------------------------------------------------------------------
class Scene:
    """A 360 x 181 full-sky CAR map with a random IQU sky; a boresight raster of T = 362 x 1000 samples, uniform in pixel space with
    a sub-pixel jitter, built with quat_from_radec; nine detectors at three polarisation angles (0, 60 and 120 degrees) up to a
    degree off the boresight, with efficiencies gamma in [0.8, 1] and one weight per detector."""

    def __init__(self, pj, dev):
        self.shape, self.wcs = N.geometries(pj)["cc_360x181"]
        rng = np.random.default_rng(416)
        rows, cols = 362, 1000
        self.nt, self.nd = rows * cols, 9
        x = (np.arange(cols)[None, :] + rng.uniform(0, 1, (rows, cols))) * (360.0 / cols) - 180.0
        y = (np.arange(rows)[:, None] + rng.uniform(0, 1, (rows, cols))) * (181.0 / rows) - 90.5
        y = np.clip(y, -90.0, 90.0)
        deg = np.pi / 180
        qb = pj.quat_from_radec(torch.from_numpy(x.reshape(-1) * deg), torch.from_numpy(y.reshape(-1) * deg),
                                torch.from_numpy(rng.uniform(-0.2, 0.2, self.nt)))
        xi, eta = rng.uniform(-1, 1, 9) * deg, rng.uniform(-1, 1, 9) * deg
        psi = np.repeat([0.0, 60.0, 120.0], 3) * deg
        centre = pj.quat_from_radec(0.0, 0.0, 0.0)
        qd = pj.quat_mul(pj.quat_conj(centre), pj.quat_from_radec(torch.from_numpy(xi), torch.from_numpy(eta), torch.from_numpy(psi)))
        self.q_bore, self.q_det = qb.to(dev).contiguous(), qd.to(dev).contiguous()
        self.gamma = to_dev(rng.uniform(0.8, 1.0, 9), dev)
        self.w = to_dev(10.0 ** rng.uniform(-1, 1, 9), dev)
        self.m0 = rng.normal(size=(3, self.shape[1], self.shape[0]))
        self.sky, self.resp = pj.expand_pointing(self.q_bore, self.q_det, self.gamma)
        m0 = pj.Enmap(to_dev(self.m0, dev), self.wcs)
        self.tod0 = pj.sample_pol_nearest(m0, self.sky, self.resp).reshape(self.nd, self.nt)
        self.tod1 = pj.sample_pol(m0, self.sky, self.resp).reshape(self.nd, self.nt)
        self.w_all = self.w[:, None].expand(self.nd, self.nt).reshape(-1).contiguous()
        self.hits = pj.scatter_nearest(torch.ones_like(self.w_all), self.sky, self.shape, self.wcs).data.cpu().numpy().reshape(self.shape[1], self.shape[0])
        self.chunk_t = 77777                              # does not divide T = 362000: five chunks, the last one short


@pytest.fixture(scope="module")
def scene(pj, dev):
    return Scene(pj, dev)


def _accumulate(pj, scene, tod, order):
    """rhs and weights as the _tod map-makers accumulate them, through their own source of chunks."""
    from pixell_jl_amd import mapmaker
    rhs = wts = None
    for d, wc, sky, resp in mapmaker._TodChunks("test", tod, scene.w, scene.q_bore, scene.q_det, scene.gamma, scene.chunk_t).chunks():
        if order == 0:
            rhs, wts = pj.bin_pol_nearest(d, wc, sky, resp, scene.shape, scene.wcs, rhs=rhs, weights=wts)
        else:
            rhs = pj.scatter_pol(wc * d, sky, resp, scene.shape, scene.wcs, order=1, out=rhs)
            wts = pj.scatter_pol_weights(wc, sky, resp, scene.shape, scene.wcs, order=1, out=wts)
    return rhs.data.cpu().numpy(), wts.data.cpu().numpy()


def test_binned_map_from_tod_recovers_the_sky(pj, dev, scene):
    """binned_map_pol_nearest_tod of noiseless d = P m0, in chunks that do not divide T, returns m0 on every solved pixel within
    nearest_ref.map_bound -- 16 (k + 50) 2^-52 ||m0(p)||_1 / rc(p), derived in tests/test_gpu_polsolve.py and
    tests/nearest_ref.py: every sample of pixel p is (I0 + q Q0) + u U0 of the pixel's own triple with the (q, u) the expansion
    wrote, which is all the derivation uses -- and unsolved pixels are +0.0.  Against the batch form on the fully expanded
    arrays: the same solved set, maps within the same bound of m0 each, and rhs and weights within k 2^-52 S of each other (two
    atomic accumulations of the same terms: never compared by bits)."""
    s = scene
    m, rc, wts = pj.binned_map_pol_nearest_tod(s.tod0, s.w, s.q_bore, s.q_det, s.gamma, s.shape, s.wcs, rcond_min=N.RCOND_MIN, chunk_t=s.chunk_t)
    mb, rcb, wtsb = pj.binned_map_pol_nearest([(s.tod0.reshape(-1), s.w_all, s.sky, s.resp)], s.shape, s.wcs, rcond_min=N.RCOND_MIN)
    nx, ny = s.shape
    assert tuple(m.data.shape) == (3, ny, nx) and tuple(rc.data.shape) == (ny, nx) and tuple(wts.data.shape) == (6, ny, nx)
    m, rc, wts, mb, rcb, wtsb = (e.data.cpu().numpy() for e in (m, rc, wts, mb, rcb, wtsb))
    solved = rc >= N.RCOND_MIN
    print("solved %d of %d pixels (%d hit), min hits %d, mean %.1f" % (solved.sum(), solved.size, (s.hits > 0).sum(), s.hits.min(), s.hits.mean()))
    assert solved.mean() >= 0.95
    for name, mm, rr in (("tod", m, rc), ("batch", mb, rcb)):
        ok = rr >= N.RCOND_MIN
        err, b = np.abs(mm - s.m0).max(axis=0), N.map_bound(s.m0, s.hits, rr)
        print("%s: worst error / bound = %.3g, worst error %.3g, min rcond %.3g" % (name, float((err[ok] / b[ok]).max()), float(err[ok].max()), float(rr[ok].min())))
        assert np.all(err[ok] <= b[ok])
        assert not bits(mm[:, ~ok]).any()
    assert np.array_equal(solved, rcb >= N.RCOND_MIN)
    # rhs and weights, chunked against whole
    rhs_c, wts_c = _accumulate(pj, s, s.tod0, 0)
    rhs_w, wts_w = pj.bin_pol_nearest(s.tod0.reshape(-1), s.w_all, s.sky, s.resp, s.shape, s.wcs)
    v = (s.w_all * s.tod0.reshape(-1)).abs()
    S3 = pj.scatter_pol_nearest(v, s.sky, s.resp.abs(), s.shape, s.wcs).data.cpu().numpy()
    S6 = pj.scatter_pol_weights_nearest(s.w_all, s.sky, s.resp.abs(), s.shape, s.wcs).data.cpu().numpy()
    R.held(rhs_c, rhs_w.data.cpu().numpy(), np.broadcast_to(s.hits, S3.shape).astype(np.int64), S3, "rhs, chunked against whole")
    R.held(wts_c, wts_w.data.cpu().numpy(), np.broadcast_to(s.hits, S6.shape).astype(np.int64), S6, "weights, chunked against whole")
    R.held(wts, wtsb, np.broadcast_to(s.hits, S6.shape).astype(np.int64), S6, "returned weights, tod against batch")


def test_cg_map_from_tod_converges(pj, dev, scene):
    """The same scene at order 1: cg_map_pol_tod converges at tol = 1e-8 (the tolerance tests/test_gpu_mapmaker.py runs cg_map_pol
    at), and the TRUE residual b - A x, recomputed with the batch operators on the fully expanded arrays, meets the stopping
    rule to 1 % as test_full_sky_in_three_batches asks of cg_map_pol.  rhs and weights, chunked against whole, under k 2^-52 S
    with k bounded from above by the hits of the 3 x 3 pixels around (a bilinear term comes from a point whose nearest pixel is
    at most one away in each axis)."""
    s = scene
    tol = 1e-8
    m, rcond, info = pj.cg_map_pol_tod(s.tod1, s.w, s.q_bore, s.q_det, s.gamma, s.shape, s.wcs, rcond_min=N.RCOND_MIN, tol=tol, chunk_t=s.chunk_t)
    assert isinstance(m, pj.Enmap) and tuple(m.data.shape) == (3, s.shape[1], s.shape[0])
    d = s.tod1.reshape(-1)
    b = pj.scatter_pol(s.w_all * d, s.sky, s.resp, s.shape, s.wcs)
    weights = pj.scatter_pol_weights(s.w_all, s.sky, s.resp, s.shape, s.wcs)
    ax = pj.normal_pol(m, s.w_all, s.sky, s.resp)
    r = pj.Enmap(b.data - ax.data, s.wcs)
    rz = float(torch.dot(r.data.view(-1), pj.pol_block_solve(r, weights, rcond_min=N.RCOND_MIN).data.view(-1)))
    rz0 = float(torch.dot(b.data.view(-1), pj.pol_block_solve(b, weights, rcond_min=N.RCOND_MIN).data.view(-1)))
    rel = np.sqrt(rz / rz0)
    off = float(np.abs(m.data.cpu().numpy() - s.m0)[:, rcond.data.cpu().numpy() >= N.RCOND_MIN].max())
    print("cg from tod: %d iterations, recursive residual %.3g, true residual %.3g, max|x - m0| = %.3g" % (
        info["iterations"], info["history"][-1], rel, off))
    assert info["converged"] and not info["breakdown"]
    assert rel <= 1.01 * tol
    rhs_c, wts_c = _accumulate(pj, s, s.tod1, 1)
    hp = np.pad(s.hits, ((1, 1), (0, 0)))
    k = sum(np.roll(hp, dx, axis=1)[1 + dy:1 + dy + s.hits.shape[0]] for dx in (-1, 0, 1) for dy in (-1, 0, 1)).astype(np.int64)
    S3 = pj.scatter_pol((s.w_all * d).abs(), s.sky, s.resp.abs(), s.shape, s.wcs).data.cpu().numpy()
    S6 = pj.scatter_pol_weights(s.w_all, s.sky, s.resp.abs(), s.shape, s.wcs).data.cpu().numpy()
    R.held(rhs_c, b.data.cpu().numpy(), np.broadcast_to(k, S3.shape), S3, "order 1 rhs, chunked against whole")
    R.held(wts_c, weights.data.cpu().numpy(), np.broadcast_to(k, S6.shape), S6, "order 1 weights, chunked against whole")


def test_map_makers_refuse_what_their_batch_forms_refuse(pj, dev, scene):
    s = scene
    tod, qb = s.tod0[:, :1000].contiguous(), s.q_bore[:1000]
    for fn in (pj.binned_map_pol_nearest_tod, pj.cg_map_pol_tod):
        bad = tod.clone()
        bad[3, 17] = float("inf")
        with pytest.raises(ValueError, match="not finite"):
            fn(bad, s.w, qb, s.q_det, s.gamma, s.shape, s.wcs, chunk_t=300)
        with pytest.raises(ValueError, match="rcond_min"):
            fn(tod, s.w, qb, s.q_det, s.gamma, s.shape, s.wcs, rcond_min=0.0)
        with pytest.raises(ValueError, match="Float64"):
            fn(tod.float(), s.w, qb, s.q_det, s.gamma, s.shape, s.wcs)
        with pytest.raises(ValueError, match="w is"):
            fn(tod, s.w[:5], qb, s.q_det, s.gamma, s.shape, s.wcs)
        with pytest.raises(ValueError, match="q_bore"):
            fn(tod, s.w, s.q_bore[:999], s.q_det, s.gamma, s.shape, s.wcs)
        with pytest.raises(ValueError, match="chunk_t"):
            fn(tod, s.w, qb, s.q_det, s.gamma, s.shape, s.wcs, chunk_t=0)
        with pytest.raises(ValueError, match="CAR only"):
            fn(tod, s.w, qb, s.q_det, s.gamma, s.shape, pj.Gnomonic((-0.01, 0.01), (1.0, 1.0), (0.0, 0.0)))
    # w of shape (D, T) is the per-detector w spread over time: the same weights within the scatters' clause
    m1, _rc, w1 = pj.binned_map_pol_nearest_tod(tod, s.w, qb, s.q_det, None, s.shape, s.wcs, chunk_t=1000)
    m2, _rc, w2 = pj.binned_map_pol_nearest_tod(tod, s.w[:, None].expand(9, 1000).contiguous(), qb, s.q_det, None, s.shape, s.wcs, chunk_t=999)
    assert float((w1.data - w2.data).abs().max()) <= 1e-12 * float(w1.data.abs().max())          # a few terms of size <= 10 per pixel


# ---- argument refusals through Python -------------------------------------------------------------------------------------------------
def test_argument_refusals(pj, dev):
    qb, qd = _inputs(3, 10, "random", 5)
    qb, qd, g = to_dev(qb, dev), to_dev(qd, dev), to_dev([0.5, 0.6, 0.7], dev)
    ok = lambda **kw: pj.expand_pointing(kw.pop("qb", qb), kw.pop("qd", qd), kw.pop("g", g), **kw)
    ok()
    for kw in (dict(qb=qb.float()), dict(qd=qd.float()), dict(g=g.float()), dict(out_sky=torch.empty((30, 2), dtype=torch.float32, device=dev)),
               dict(out_resp=torch.empty((30, 2), dtype=torch.float32, device=dev))):
        with pytest.raises(ValueError, match="Float64"):
            ok(**kw)
    for kw in (dict(qb=qb[:, :3].contiguous()), dict(qb=qb.reshape(-1)), dict(qd=qd.reshape(1, 3, 4)), dict(qd=qd.t().contiguous()),
               dict(g=g[:2]), dict(g=g[:, None]), dict(out_sky=torch.empty((29, 2), dtype=torch.float64, device=dev)),
               dict(out_resp=torch.empty((31, 2), dtype=torch.float64, device=dev)), dict(out_sky=torch.empty((2, 30), dtype=torch.float64, device=dev))):
        with pytest.raises(ValueError):
            ok(**kw)
    wide = torch.empty((30, 4), dtype=torch.float64, device=dev)
    for kw in (dict(qb=torch.empty((10, 8), dtype=torch.float64, device=dev)[:, :4]), dict(qd=torch.empty((3, 8), dtype=torch.float64, device=dev)[:, ::2]),
               dict(g=torch.empty(6, dtype=torch.float64, device=dev)[::2]), dict(out_sky=wide[:, :2]), dict(out_resp=wide[:, 2:])):
        with pytest.raises(ValueError, match="contiguous"):
            ok(**kw)
    for kw in (dict(qb=qb.cpu()), dict(qd=qd.cpu()), dict(g=g.cpu())):
        with pytest.raises((RuntimeError, ValueError)):
            ok(**kw)
    if torch.cuda.device_count() > 1:
        other = torch.device("cuda:1")
        for kw in (dict(qd=qd.to(other)), dict(g=g.to(other)), dict(out_sky=torch.empty((30, 2), dtype=torch.float64, device=other))):
            with pytest.raises(ValueError):
                ok(**kw)
    # overlaps: an output on an input, and the two outputs on each other
    big = torch.zeros((40, 4), dtype=torch.float64, device=dev)
    qb_in = big[:10]
    both = torch.empty((45, 2), dtype=torch.float64, device=dev)
    for kw in (dict(qb=qb_in, out_sky=big.view(-1, 2)[:30]), dict(qb=qb_in, out_resp=big.view(-1, 2)[10:40]),
               dict(out_sky=both[:30], out_resp=both[15:])):
        with pytest.raises(ValueError, match="overlap"):
            ok(**kw)
    a, b = ok(out_sky=both[:30], out_resp=torch.empty((30, 2), dtype=torch.float64, device=dev))
    assert a.data_ptr() == both.data_ptr()
    with pytest.raises(TypeError):
        pj.expand_pointing(qb.cpu().numpy(), qd)
