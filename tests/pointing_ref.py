"""The numpy yardstick of detector pointing expansion: the definition of include/pixell_hip.h's
pxl_pointing_expand_f64 written out literally -- rotate z^ and x^, build east and north, project -- in ONE function parameterised
by dtype.  np.float64 is the yardstick (what a careful user would write with libm); np.longdouble (80-bit here) is the truth.
Nothing here is the closed form the kernel evaluates (pxl_pointing.h): agreement of the two is what the tests check.

Error measures, both against the truth and never per coordinate:
  position   the great-circle separation of the two (ra, dec), in units of 2^-52 rad (ra alone is ill-conditioned as 1 / h and
             jumps by 2 pi at the branch cut)
  response   max(|dq|, |du|) in units of 2^-52 gamma / h, h = sin of the colatitude of the truth: the 1 / h is the conditioning
             of a position angle next to a pole"""
import numpy as np

EPS = 2.0 ** -52


def quat_mul(a, b):
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), axis=-1)


def quat_conj(q):
    return q * np.array([1, -1, -1, -1], dtype=q.dtype)


def quat_from_radec(ra, dec, psi, dtype=np.float64):
    """Rz(ra) (x) Ry(pi/2 - dec) (x) Rz(pi - psi)"""
    ra, dec, psi = np.broadcast_arrays(*(np.asarray(v, dtype=dtype) for v in (ra, dec, psi)))
    pi = np.arctan2(dtype(0), dtype(-1))
    zero = np.zeros_like(ra)

    def rz(a):
        return np.stack((np.cos(a / 2), zero, zero, np.sin(a / 2)), axis=-1)

    tilt = (pi / 2 - dec) / 2
    ry = np.stack((np.cos(tilt), zero, np.sin(tilt), zero), axis=-1)
    return quat_mul(quat_mul(rz(ra), ry), rz(pi - psi))


def expand_pairs(qb, qd, gamma=None, dtype=np.float64):
    """The definition for n (boresight, detector) pairs: qb, qd (n, 4), gamma (n,) or None.  Returns a dict of (n,) arrays of
    `dtype`: ra, dec, q, u, h (of the unit line of sight) and nx (the unnormalised n_x, for the tests of the pole rule)."""
    qb, qd = np.asarray(qb, dtype=np.float64), np.asarray(qd, dtype=np.float64)
    g64 = np.ones(qb.shape[0]) if gamma is None else np.asarray(gamma, dtype=np.float64)
    bad = ~(np.isfinite(qb).all(-1) & np.isfinite(qd).all(-1) & np.isfinite(g64)) | (qb == 0).all(-1) | (qd == 0).all(-1)
    with np.errstate(all="ignore"):
        q = quat_mul(np.where(bad[:, None], 1.0, qb).astype(dtype), np.where(bad[:, None], 1.0, qd).astype(dtype))
        g = np.where(bad, 1.0, g64).astype(dtype)
        w, x, y, z = (q[:, i] for i in range(4))
        two = dtype(2)
        # S R(q) z^ and S R(q) x^, S = |q|^2
        n = np.stack((two * (x * z + w * y), two * (y * z - w * x), w * w - x * x - y * y + z * z), axis=-1)
        e = np.stack((w * w + x * x - y * y - z * z, two * (x * y + w * z), two * (x * z - w * y)), axis=-1)
        h = np.sqrt(n[:, 0] ** 2 + n[:, 1] ** 2)
        pole = h == 0
        ra = np.where(pole, dtype(0), np.arctan2(n[:, 1] + dtype(0), n[:, 0]))        # + 0: -0.0 -> +0.0, so never -pi
        dec = np.arctan2(n[:, 2], h)
        nhat = n / np.sqrt((n * n).sum(-1))[:, None]
        hs = np.where(pole, dtype(1), h)
        east = np.stack((np.where(pole, dtype(0), -n[:, 1] / hs), np.where(pole, dtype(1), n[:, 0] / hs), np.zeros_like(h)), axis=-1)
        north = np.cross(nhat, east)
        c, s = (e * north).sum(-1), (e * east).sum(-1)
        d = c * c + s * s
        out = {"ra": ra, "dec": dec, "q": g * (c * c - s * s) / d, "u": g * (two * c * s) / d, "h": h / np.sqrt((n * n).sum(-1)),
               "nx": n[:, 0]}
    for k in out:
        out[k] = np.where(bad, dtype(np.nan), out[k])
    return out


def expand(q_bore, q_det, gamma=None, dtype=np.float64):
    """The (T, 4) x (D, 4) form, detector-major: sample k = d * T + t."""
    q_bore, q_det = np.asarray(q_bore, dtype=np.float64), np.asarray(q_det, dtype=np.float64)
    nt, nd = q_bore.shape[0], q_det.shape[0]
    g = None if gamma is None else np.repeat(np.asarray(gamma, dtype=np.float64), nt)
    return expand_pairs(np.tile(q_bore, (nd, 1)), np.repeat(q_det, nt, axis=0), g, dtype)


def separation(ra, dec, truth):
    """Great-circle separation of (ra, dec) from the truth's, in units of 2^-52 rad, evaluated in long double from the chord."""
    L = np.longdouble

    def vec(a, d):
        a, d = np.asarray(a, dtype=L), np.asarray(d, dtype=L)
        return np.stack((np.cos(d) * np.cos(a), np.cos(d) * np.sin(a), np.sin(d)), axis=-1)

    chord = np.sqrt(((vec(ra, dec) - vec(truth["ra"], truth["dec"])) ** 2).sum(-1))
    return (2 * np.arcsin(chord / 2) / L(EPS)).astype(np.float64)


def response_error(q, u, truth, gamma=None):
    """max(|dq|, |du|) in units of 2^-52 gamma / h.  Where gamma is 0 the response must be 0: any other value counts as inf."""
    L = np.longdouble
    g = np.ones(len(truth["h"]), dtype=L) if gamma is None else np.asarray(gamma, dtype=L)
    err = np.maximum(np.abs(np.asarray(q, dtype=L) - truth["q"]), np.abs(np.asarray(u, dtype=L) - truth["u"]))
    with np.errstate(all="ignore"):
        units = err * truth["h"].astype(L) / (L(EPS) * np.abs(g))
    return np.where(g == 0, np.where(err == 0, 0.0, np.inf), units).astype(np.float64)


def worst(got, truth, gamma=None):
    """(worst position error, worst response error) of got = {ra, dec, q, u} over the samples the truth defines (not NaN)."""
    ok = ~np.isnan(truth["ra"].astype(np.float64))
    t = {k: v[ok] for k, v in truth.items()}
    g = None if gamma is None else np.asarray(gamma)[ok]
    return (float(separation(got["ra"][ok], got["dec"][ok], t).max()), float(response_error(got["q"][ok], got["u"][ok], t, g).max()))


# ---- the input families the tests share ----------------------------------------------------------------------------------

def random_quats(rng, n):
    """n quaternions uniform in direction with norms from 0.5 to 2"""
    q = rng.standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1)[:, None] * rng.uniform(0.5, 2.0, n)[:, None]


def polar_quats(rng, n, hmin=1e-12, hmax=1e-1):
    """n boresight quaternions looking within h of a pole, h log-uniform in [hmin, hmax], both poles, norms from 0.5 to 2"""
    h = np.exp(rng.uniform(np.log(hmin), np.log(hmax), n))
    dec = np.where(rng.random(n) < 0.5, 1.0, -1.0) * (np.pi / 2 - h)
    q = quat_from_radec(rng.uniform(-np.pi, np.pi, n), dec, rng.uniform(-np.pi, np.pi, n))
    return q * rng.uniform(0.5, 2.0, n)[:, None]


def polar_sign_patterns():
    """The 32 boresights (+-1, +-0, +-0, +-1) (north pole) and (+-0, +-1, +-1, +-0) (south pole): every signed zero n_x and n_y can be."""
    out = []
    for bits in range(16):
        sg = [-1.0 if bits >> i & 1 else 1.0 for i in range(4)]
        out.append([sg[0] * 1.0, sg[1] * 0.0, sg[2] * 0.0, sg[3] * 1.0])
        out.append([sg[0] * 0.0, sg[1] * 1.0, sg[2] * 1.0, sg[3] * 0.0])
    return np.array(out)
