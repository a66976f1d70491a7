"""tests/pointing_ref.py, the numpy yardstick of detector pointing expansion, checked on its own: against an
independent route through scipy's Rotation, through the quat_from_radec round trip that fixes the convention, on the pole
rule, on scale invariance and on the NaN / Inf / zero rule.  Also the package's host helpers (pj.quat_from_radec, quat_mul,
quat_conj: torch, no kernel) against it.  No GPU."""
import numpy as np
import pytest

import pointing_ref as ref

L = np.longdouble


@pytest.fixture(scope="module")
def pairs():
    rng = np.random.default_rng(416)
    n = 20000
    qb = np.concatenate((ref.random_quats(rng, n), ref.polar_quats(rng, n // 4)))
    qd = ref.random_quats(rng, len(qb))
    qd[n:] = [1.0, 0.0, 0.0, 0.0]                       # the polar set looks where the boresight looks
    return qb, qd


def test_float64_against_long_double(pairs):
    """The yardstick's own error: measured 2.75 (position, 2^-52 rad) and 4.74 (response units) on 2e5 random pairs when the
    feature was specified; the bound here is four times that -- a yardstick that needed more would be no yardstick."""
    qb, qd = pairs
    pos, resp = ref.worst(ref.expand_pairs(qb, qd), ref.expand_pairs(qb, qd, dtype=L))
    print("float64 yardstick against long double: position %.2f x 2^-52 rad, response %.2f units" % (pos, resp))
    assert pos <= 4 * 2.75 and resp <= 4 * 4.74


def test_against_scipy_rotation(pairs):
    """An independent route: scipy normalises the quaternion and rotates z^ and x^; the position angle comes from atan2 of the
    components along east and north built with numpy's cross products, the declination from asin away from the poles."""
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    qb, qd = pairs
    q = ref.quat_mul(qb, qd)
    rot = Rotation.from_quat(q[:, [1, 2, 3, 0]])         # scipy is scalar-last
    n, e = rot.apply([0.0, 0.0, 1.0]), rot.apply([1.0, 0.0, 0.0])
    east = np.cross([0.0, 0.0, 1.0], n)
    h = np.linalg.norm(east, axis=1)
    east /= h[:, None]
    north = np.cross(n, east)
    psi = np.arctan2((e * east).sum(1), (e * north).sum(1))
    got = ref.expand_pairs(qb, qd)
    sep = ref.separation(np.arctan2(n[:, 1], n[:, 0]), np.arctan2(n[:, 2], h), {"ra": got["ra"], "dec": got["dec"]})
    assert sep.max() <= 16, sep.max()                    # two Float64 routes, each a few 2^-52 from the truth
    away = np.abs(n[:, 2]) < 0.9
    assert np.abs(np.arcsin(n[away, 2]) - got["dec"][away]).max() <= 16 * ref.EPS
    err = np.maximum(np.abs(np.cos(2 * psi) - got["q"]), np.abs(np.sin(2 * psi) - got["u"])) * h / ref.EPS
    assert err.max() <= 32, err.max()                    # units of 2^-52 / h; two routes of ~5 units each and the 2 psi of a rounded psi


def test_quat_from_radec_round_trip():
    """expand(quat_from_radec(ra, dec, psi), identity) = (ra, dec), (cos 2 psi, sin 2 psi): the convention, in closed form.
    Declinations within 1e-12 of both poles included; measured 7e-16 rad and 2.1e-15 when the feature was specified."""
    rng = np.random.default_rng(7)
    n = 20000
    ra, psi = rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n)
    dec = np.arcsin(rng.uniform(-1, 1, n))
    dec[: n // 4] = np.where(rng.random(n // 4) < 0.5, 1, -1) * (np.pi / 2 - np.exp(rng.uniform(np.log(1e-12), np.log(1e-1), n // 4)))
    ident = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    got = ref.expand_pairs(ref.quat_from_radec(ra, dec, psi), ident)
    sep = ref.separation(got["ra"], got["dec"], {"ra": ra, "dec": dec}) * ref.EPS
    h = np.cos(dec)
    err = np.maximum(np.abs(got["q"] - np.cos(2 * psi)), np.abs(got["u"] - np.sin(2 * psi)))
    print("round trip: separation %.2e rad, response %.2e (times h: %.2e)" % (sep.max(), err.max(), (err * h).max()))
    assert sep.max() <= 2e-15
    # the response's error carries the 1 / h of a position angle: quat_from_radec rounds ra and psi into one angle near a pole
    assert (err * np.maximum(h, 1e-3)).max() <= 1e-14 and err[h > 0.1].max() <= 1e-14
    # a detector offset: q_det = conj(q_b) (x) q_d looks at (ra_d, dec_d, psi_d) when the boresight is q_b
    qb, qd = ref.quat_from_radec(ra, dec, psi), ref.quat_from_radec(ra[::-1], dec[::-1], psi[::-1])
    got = ref.expand_pairs(qb, ref.quat_mul(ref.quat_conj(qb), qd))
    assert (ref.separation(got["ra"], got["dec"], {"ra": ra[::-1], "dec": dec[::-1]}) * ref.EPS).max() <= 4e-15


def test_position_angle_is_from_north_through_east():
    """At (ra, dec) = (0, 0) north is +z and east is +y: psi = 0 points the sensitive direction north, psi = pi/2 east."""
    for psi, want in ((0.0, [0, 0, 1]), (np.pi / 2, [0, 1, 0])):
        q = ref.quat_from_radec(0.0, 0.0, psi)[None]
        w, x, y, z = q[0]
        e = np.array([w * w + x * x - y * y - z * z, 2 * (x * y + w * z), 2 * (x * z - w * y)])
        assert np.allclose(e, want, atol=1e-15)
        got = ref.expand_pairs(q, np.array([[1.0, 0, 0, 0]]))
        assert np.allclose([got["q"][0], got["u"][0]], [np.cos(2 * psi), np.sin(2 * psi)], atol=1e-15)


def test_pole_rule():
    """h == 0: ra = +0.0 by bits (also where n_x = -0.0, for which atan2 alone answers pi), dec = +-pi/2, E = (0, 1, 0)."""
    ident = np.array([[1.0, 0, 0, 0]])
    for dtype in (np.float64, L):
        # north: q = (w, 0, 0, z) is Rz(a), e = (cos a, sin a, 0), N = (-1, 0, 0): c = -cos a, s = sin a, psi = pi - a
        for a in (0.0, 0.3, -2.0):
            q = np.array([[np.cos(a / 2), 0.0, 0.0, np.sin(a / 2)]]) * 1.5
            got = ref.expand_pairs(q, ident, dtype=dtype)
            assert got["ra"][0] == 0 and not np.signbit(got["ra"][0]) and abs(got["dec"][0] - np.pi / 2) < 1e-15
            assert np.allclose([float(got["q"][0]), float(got["u"][0])], [np.cos(2 * (np.pi - a)), np.sin(2 * (np.pi - a))], atol=1e-15)
        # south: q = (0, 1, 0, 0) is the half turn about x^: n = -z^
        got = ref.expand_pairs(np.array([[0.0, 1.0, 0.0, 0.0]]), ident, dtype=dtype)
        assert got["ra"][0] == 0 and not np.signbit(got["ra"][0]) and abs(got["dec"][0] + np.pi / 2) < 1e-15
        # every signed-zero form of a polar boresight, (+-1, +-0, +-0, +-1) and (+-0, +-1, +-1, +-0): some give n_x = -0.0, for which atan2
        # alone answers pi
        q = ref.polar_sign_patterns()
        got = ref.expand_pairs(q, np.tile(ident, (len(q), 1)), dtype=dtype)
        assert (np.signbit(got["nx"]) & (got["nx"] == 0)).any() and not (got["nx"] != 0).any()
        assert (got["ra"] == 0).all() and not np.signbit(got["ra"]).any() and (np.abs(got["dec"]) > 1.57).all()
    # off the pole ra = pi is reached and -pi is not: n_y = -0.0 with n_x < 0
    q = np.array([[1.0, 0.0, -1.0, -0.0]])               # n = (-2, -0.0 - 0.0, 0)
    got = ref.expand_pairs(q, ident)
    assert got["ra"][0] == np.pi


def test_scale_invariance(pairs):
    qb, qd = pairs
    rng = np.random.default_rng(3)
    truth = ref.expand_pairs(qb, qd, dtype=L)
    sb, sd = rng.uniform(0.5, 2.0, len(qb)), rng.uniform(0.5, 2.0, len(qb))
    nb, nd = np.linalg.norm(qb, axis=1), np.linalg.norm(qd, axis=1)
    scaled = ref.expand_pairs(qb * (sb / nb)[:, None], qd * (sd / nd)[:, None], dtype=L)
    # the scaled inputs are rounded to Float64 again: each component moves by 2^-53 relative, the direction by a few 2^-52
    pos, resp = ref.worst({k: scaled[k].astype(np.float64) for k in scaled}, truth)
    assert pos <= 8 and resp <= 16, (pos, resp)
    # a power of two is exact: the same bits
    for f in (0.5, 2.0):
        a, b = ref.expand_pairs(qb, qd), ref.expand_pairs(qb * f, qd / f * 2)
        for k in ("ra", "dec", "q", "u"):
            assert np.array_equal(a[k], b[k])


def test_nan_inf_and_zero_rule():
    rng = np.random.default_rng(5)
    qb, qd = ref.random_quats(rng, 40), ref.random_quats(rng, 40)
    gamma = rng.uniform(0, 1, 40)
    clean = ref.expand_pairs(qb, qd, gamma)
    bad = {}
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        for c in range(4):
            qb[4 * k + c, c] = v
            qd[12 + 4 * k + c, c] = v
            bad[4 * k + c] = bad[12 + 4 * k + c] = True
    qb[24], qd[25], gamma[26], gamma[27] = 0.0, [0.0, -0.0, 0.0, 0.0], np.nan, np.inf
    bad.update({24: True, 25: True, 26: True, 27: True})
    gamma[28] = 0.0                                      # a dead detector is not a cut: its response is 0, its position stands
    for dtype in (np.float64, L):
        got = ref.expand_pairs(qb, qd, gamma, dtype=dtype)
        for i in range(40):
            vals = [got[k][i] for k in ("ra", "dec", "q", "u")]
            assert all(np.isnan(v) for v in vals) if i in bad else all(np.isfinite(v) for v in vals), (i, vals)
    got = ref.expand_pairs(qb, qd, gamma)
    keep = [i for i in range(40) if i not in bad and i != 28]
    for k in ("ra", "dec", "q", "u"):
        assert np.array_equal(got[k][keep], clean[k][keep])
    assert got["q"][28] == 0 and got["u"][28] == 0 and got["ra"][28] == clean["ra"][28]


def test_detector_major_layout():
    rng = np.random.default_rng(9)
    qb, qd, gamma = ref.random_quats(rng, 5), ref.random_quats(rng, 3), rng.uniform(0, 1, 3)
    full = ref.expand(qb, qd, gamma)
    for d in range(3):
        for t in range(5):
            one = ref.expand_pairs(qb[t:t + 1], qd[d:d + 1], gamma[d:d + 1])
            assert all(one[k][0] == full[k][d * 5 + t] for k in ("ra", "dec", "q", "u"))


def test_package_host_helpers_agree(pj):
    """pj.quat_from_radec, quat_mul and quat_conj (torch on the host) are the yardstick's, to Float64 rounding."""
    import torch
    rng = np.random.default_rng(11)
    ra, dec, psi = rng.uniform(-np.pi, np.pi, 100), rng.uniform(-np.pi / 2, np.pi / 2, 100), rng.uniform(-np.pi, np.pi, 100)
    q = pj.quat_from_radec(torch.from_numpy(ra), torch.from_numpy(dec), torch.from_numpy(psi))
    assert q.shape == (100, 4) and q.dtype == torch.float64
    assert np.abs(q.numpy() - ref.quat_from_radec(ra, dec, psi)).max() <= 4 * ref.EPS
    a, b = ref.random_quats(rng, 100), ref.random_quats(rng, 100)
    assert np.array_equal(pj.quat_mul(torch.from_numpy(a), torch.from_numpy(b)).numpy(), ref.quat_mul(a, b))
    assert np.array_equal(pj.quat_conj(torch.from_numpy(a)).numpy(), ref.quat_conj(a))
    assert pj.quat_from_radec(0.1, 0.2, 0.3).shape == (4,)
