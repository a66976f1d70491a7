"""Brute-force yardstick for distance_transform, transform_distance.jl:55-78 step for step in numpy: the pixel centres'
RA / DEC as :56-57 take them (pix2sky over 1:nx and 1:ny with the per-element rewind: the oracle's PXL_WRAP_REWIND), the
list of zero pixels (:59-64, iszero), for every pixel the squared chord to every zero in `metric`'s difference form
(:81-92), the minimum, acos(1 - d2/2).  The sampled form takes a list of pixels and an explicit list of zeros, for maps too
large for the full table.  Also the per-pixel error bound the device is held to and seeded masks."""
import math

import numpy as np

from oracle import oracle as O

EPS = 2.0 ** -52


def sky_angles(wcs, shape):
    """(alphas, deltas) of transform_distance.jl:56-57."""
    nx, ny = int(shape[0]), int(shape[1])
    ra = O.pix2sky(wcs, np.column_stack([np.arange(1, nx + 1, dtype=float), np.ones(nx)]), O.WRAP_REWIND)[:, 0]
    dec = O.pix2sky(wcs, np.column_stack([np.ones(ny), np.arange(1, ny + 1, dtype=float)]), O.WRAP_REWIND)[:, 1]
    return ra, dec


def _tables(wcs, shape):
    ra, dec = sky_angles(wcs, shape)
    return np.cos(ra), np.sin(ra), np.cos(dec), np.sin(dec)


def _d2(t, i1, j1, i2, j2):
    """metric(): x = cos(d) cos(a), y = cos(d) sin(a), z = sin(d); (x1 - x2)^2 + (y1 - y2)^2 + (z1 - z2)^2, left to right."""
    ca, sa, cd, sd = t
    x1, y1, z1 = cd[j1] * ca[i1], cd[j1] * sa[i1], sd[j1]
    x2, y2, z2 = cd[j2] * ca[i2], cd[j2] * sa[i2], sd[j2]
    return (x1 - x2) ** 2 + (y1 - y2) ** 2 + (z1 - z2) ** 2


def sampled(wcs, shape, ii, jj, zi, zj, cap=None, chunk=256):
    """Distances of the pixels (ii, jj) (0-based column, row) to the nearest of the zeros (zi, zj).  cap: optional per-pixel
    upper bound on that distance; then only zeros whose DEC lies within it of the pixel's are scanned (|DEC difference| never
    exceeds the angular distance), which leaves the minimum unchanged.  inf where no zero is listed."""
    t = _tables(wcs, shape)
    _, dec = sky_angles(wcs, shape)
    ii, jj = np.asarray(ii, dtype=np.int64), np.asarray(jj, dtype=np.int64)
    zi, zj = np.asarray(zi, dtype=np.int64), np.asarray(zj, dtype=np.int64)
    out = np.full(ii.size, np.inf)
    if zi.size == 0:
        return out
    if cap is None:
        for s in range(0, ii.size, chunk):
            d2 = _d2(t, ii[s:s + chunk, None], jj[s:s + chunk, None], zi[None, :], zj[None, :])
            out[s:s + chunk] = np.arccos(1 - d2.min(axis=1) / 2)
        return out
    ra, _ = sky_angles(wcs, shape)
    order = np.argsort(dec[zj], kind="stable")
    zi, zj = zi[order], zj[order]
    zdec, zra = dec[zj], ra[zi]
    for k in range(ii.size):
        rho, dk = cap[k] + 1e-9, dec[jj[k]]
        lo, hi = np.searchsorted(zdec, [dk - rho, dk + rho], side="left")
        if hi <= lo:
            continue
        ci, cj = zi[lo:hi], zj[lo:hi]
        if abs(dk) + rho < math.pi / 2 - 1e-6:     # a cap that misses both poles spans asin(sin rho / cos dec) either way in RA
            h = math.asin(min(1.0, math.sin(rho) / math.cos(dk))) + 1e-9
            near = np.abs(np.remainder(zra[lo:hi] - ra[ii[k]] + math.pi, 2 * math.pi) - math.pi) <= h
            ci, cj = ci[near], cj[near]
        d2 = _d2(t, ii[k], jj[k], ci, cj)
        out[k] = np.arccos(np.array([1 - d2.min() / 2]))[0]
    return out


def distance_transform(m, wcs):
    """m: (ny, nx) host array.  The reference's BruteForceSDT result (ny, nx), or None where it raises (no zero pixel)."""
    ny, nx = m.shape
    zj, zi = np.nonzero(m == 0)
    if zi.size == 0:
        return None
    jj, ii = np.divmod(np.arange(nx * ny), nx)
    return sampled(wcs, (nx, ny), ii, jj, zi, zj).reshape(ny, nx)


def bound(theta):
    """Per-pixel bound on |theta_device - theta_ref|.  In the chord d = 2 sin(theta/2):
    (i) the device's cos / sin tables against the host's: within 1 ulp each, so <= 4 eps d in d^2;
    (ii) the choice of the zero in the dot-product form: <= 4 eps absolute in d^2 (a near-tie may pick the other zero);
    (iii) the rounding of 1 - d^2/2 before acos, 1.1e-16 on each side; acos itself, 1 ulp on each side.
    theta moves by 1 / sin(theta) per unit of 1 - d^2/2, so the bound is (2 eps (1 + d) + 2.2e-16) / sin(theta) + 2 ulp;
    it is never looser than the ceiling 4e-15 / max(sin theta, 1e-3) + 8 ulp(theta)."""
    theta = np.asarray(theta, dtype=float)
    s = np.sin(theta)
    d = 2 * np.sin(theta / 2)
    with np.errstate(divide="ignore"):
        derived = (2 * EPS * (1 + d) + 2.2e-16) / s + 2 * np.spacing(theta)
    ceiling = 4e-15 / np.maximum(s, 1e-3) + 8 * np.spacing(theta)
    return np.minimum(np.where(s > 0, derived, np.inf), ceiling)


def worst_ratio(got, ref):
    """max |got - ref| / bound(ref) over the pixels (0 if all agree)."""
    err = np.abs(np.asarray(got, dtype=float) - np.asarray(ref, dtype=float))
    return float((err / bound(ref)).max()) if err.size else 0.0


def disk_zeros(wcs, shape, ncent, radius, seed):
    """(zi, zj) of a point-source mask: every pixel whose centre lies within `radius` of one of `ncent` seeded centres drawn
    uniformly on the sphere (only the rows within `radius` of a centre are scanned)."""
    nx, ny = int(shape[0]), int(shape[1])
    ca, sa, cd, sd = _tables(wcs, shape)
    _, dec = sky_angles(wcs, shape)
    rng = np.random.default_rng(seed)
    zc = rng.uniform(-1.0, 1.0, ncent)
    ac = rng.uniform(-math.pi, math.pi, ncent)
    dc = np.arcsin(zc)
    ra, _ = sky_angles(wcs, shape)
    out_i, out_j = [], []
    cr = math.cos(radius)
    for k in range(ncent):
        rows = np.nonzero(np.abs(dec - dc[k]) <= radius + 1e-12)[0]
        if rows.size == 0:
            continue
        cols = np.arange(nx)
        if abs(dc[k]) + radius < math.pi / 2 - 1e-6:       # the cap misses both poles: its RA half-width is asin(sin r / cos d)
            h = math.asin(min(1.0, math.sin(radius) / math.cos(dc[k]))) + 1e-9
            cols = np.nonzero(np.abs(np.remainder(ra - ac[k] + math.pi, 2 * math.pi) - math.pi) <= h)[0]
        cosang = (sd[rows, None] * math.sin(dc[k])
                  + cd[rows, None] * math.cos(dc[k]) * (ca[None, cols] * math.cos(ac[k]) + sa[None, cols] * math.sin(ac[k])))
        r, c = np.nonzero(cosang >= cr)
        out_j.append(rows[r])
        out_i.append(cols[c])
    if not out_i:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    z = np.unique(np.concatenate(out_j) * nx + np.concatenate(out_i))
    return z % nx, z // nx


def band_rows(wcs, shape, halfwidth):
    """Rows of the band |DEC| < halfwidth."""
    _, dec = sky_angles(wcs, shape)
    return np.nonzero(np.abs(dec) < halfwidth)[0]
