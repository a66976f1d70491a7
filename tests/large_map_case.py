"""Bands of rows and point batches for maps whose flat element offsets pass 2^29, 2^31 and 2^32, numpy only.

A (nc, ny, nx) map is far too large for a dense yardstick, and none is needed: the yardsticks of tests/*_ref.py compute every
position on the FULL geometry and index a resident window of rows (row0, nrows).  This module derives, from a shape alone, the
windows worth holding resident and the points that read and write them.  Nothing is typed in.

  thresholds  element offsets 2^29 (byte offsets pass 4 GiB), 2^31 (an int product goes negative) and 2^32, counted across the
              planes: element (c, r, i) sits at c * ny * nx + r * nx + i (all 0-based).
  bands       for each threshold T below nc * ny * nx: the plane c = T // (ny * nx), the row r = (T % (ny * nx)) // nx and the
              column i = T % nx of the crossing element, and rows [r - 8, r + 8) around it; always the first 8 and the last 8
              rows of the map.  Bands do not overlap (asserted).  A band is rows of EVERY plane: the crossing lies in plane c.
  points      per band, pixel positions turned into (ra, dec) by O.pix2sky: uniform over the band's inner rows and every column;
              pixel centres and pixel edges (the order-0 ties); the columns either side of the RA seam (of the side edges on a map
              that is not periodic); the pixels either side of the crossing element; positions past the side edges; and, for the
              bands that touch them, positions before the first and past the last row of the map.  The inner rows leave two rows
              on an interior side, so the sixteen taps of order 3 stay in the band too.
  offsets     per band, plane and order, the smallest and largest flat element offset a tap reaches.

Case checks at construction that every tap of every order lies in its own band or off the map altogether (tap_ref.window
raises otherwise), so a banded yardstick never loses a tap."""
import math

import numpy as np

import nearest_ref
import scatter_cubic_ref
import scatter_ref
import tap_ref

THRESHOLDS = (("2^29", 1 << 29), ("2^31", 1 << 31), ("2^32", 1 << 32))
HALF = 8                      # rows either side of a crossing row; the first and last band have HALF rows
INNER = 2                     # rows a point keeps from an interior side of its band: order 3 reads rows j0 - 1 .. j0 + 2
N_UNIFORM, N_LATTICE = 400, 60


class Band:
    def __init__(self, name, row0, nrows, threshold=None, plane=None, cross=None):
        self.name, self.row0, self.nrows, self.threshold, self.plane, self.cross = name, row0, nrows, threshold, plane, cross

    @property
    def rows(self):
        return slice(self.row0, self.row0 + self.nrows)

    def __repr__(self):
        return "Band(%s: rows [%d, %d)%s)" % (self.name, self.row0, self.row0 + self.nrows,
                                              "" if self.threshold is None else ", plane %d, crossing at row %d column %d"
                                              % ((self.plane,) + self.cross))


def bands(shape, nc):
    """The bands of a (nc, ny, nx) map, first rows, then one per threshold crossed, then last rows."""
    nx, ny = int(shape[0]), int(shape[1])
    assert ny >= 4 * HALF
    plane = nx * ny
    out = [Band("first", 0, HALF, plane=0)]
    for name, t in THRESHOLDS:
        if t < nc * plane:
            c, r, i = t // plane, (t % plane) // nx, t % nx
            lo = min(max(r - HALF, 0), ny - 2 * HALF)
            out.append(Band(name, lo, 2 * HALF, t, c, (r, i)))
    out.append(Band("last", ny - HALF, HALF, plane=nc - 1))
    order = sorted(out, key=lambda b: b.row0)
    for a, b in zip(order, order[1:]):
        assert a.row0 + a.nrows <= b.row0, "bands overlap: %r and %r" % (a, b)
    return out


def band_pixels(shape, band, rng):
    """(n, 2) pixel positions (x, y), 1-based, for one band."""
    nx, ny = int(shape[0]), int(shape[1])
    first, last = band.row0 == 0, band.row0 + band.nrows == ny
    y_min = 0.5 if first else band.row0 + 1.0 + INNER
    y_max = ny + 0.5 if last else float(band.row0 + band.nrows - INNER)
    ry = lambda n: rng.uniform(y_min, y_max, n)
    pts = [np.stack([rng.uniform(0.5, nx + 0.5, N_UNIFORM), ry(N_UNIFORM)], axis=1)]
    # pixel centres and pixel edges: integers and half-integers inside [y_min, y_max]
    jc = rng.integers(math.ceil(y_min), math.floor(y_max) + 1, N_LATTICE)
    je = rng.integers(math.ceil(y_min - 0.5), math.floor(y_max - 0.5) + 1, N_LATTICE) + 0.5
    ic = rng.integers(1, nx + 1, N_LATTICE)
    pts += [np.stack([ic, jc], axis=1).astype(float), np.stack([ic + 0.5, je], axis=1), np.stack([ic + 0.5, jc], axis=1),
            np.stack([ic.astype(float), je], axis=1)]
    # the seam (or side-edge) columns, and beyond the side edges
    xs = np.array([0.5, 0.75, 1.0, 1.25, 1.5, nx - 0.5, nx - 0.25, nx, nx + 0.25, nx + 0.5])
    beyond = np.array([-3.2, -0.7, 0.2, nx + 0.8, nx + 2.6, nx + 40.3])
    for x in (xs, beyond):
        xx = np.repeat(x, 4)
        pts.append(np.stack([xx, ry(len(xx))], axis=1))
        pts.append(np.stack([x, rng.integers(math.ceil(y_min), math.floor(y_max) + 1, len(x)).astype(float)], axis=1))
    if band.cross is not None:
        r, i = band.cross
        dx = np.array([-2.0, -1.0, -0.5, 0.0, 0.3, 0.5, 1.0, 2.0])
        for dy in (0.0, 0.4, -0.4, 0.5, -0.5, 1.0, -1.0):
            if y_min <= r + 1 + dy <= y_max:
                pts.append(np.stack([i + 1 + dx, np.full(len(dx), r + 1 + dy)], axis=1))
    off = np.array([0.25, 0.51, 0.75, 1.5, 3.2, 40.0])
    if first:
        pts.append(np.stack([rng.uniform(0.5, nx + 0.5, 2 * len(off)), 0.5 - np.tile(off, 2)], axis=1))
    if last:
        pts.append(np.stack([rng.uniform(0.5, nx + 0.5, 2 * len(off)), ny + 0.5 + np.tile(off, 2)], axis=1))
    return np.concatenate(pts)


def order_taps(O, wcs, shape, sky, order):
    """Flat indices into the FULL (ny, nx) plane, (N, taps), -1 for no tap: order 0, 1 or 3."""
    if order == 0:
        return nearest_ref.taps(O, wcs, shape, sky)[0][:, None]
    return (scatter_ref.taps if order == 1 else scatter_cubic_ref.taps)(O, wcs, shape, sky)[0]


class Case:
    """The bands of a (nc, ny, nx) map on (shape, wcs), their points (self.sky[b], (n_b, 2) of (ra, dec)), all points in one batch
    (self.all_sky) with each band's slice of it (self.slices[b])."""

    def __init__(self, O, shape, wcs, nc, seed=0):
        self.shape, self.wcs, self.nc = (int(shape[0]), int(shape[1])), wcs, int(nc)
        self.bands = bands(self.shape, nc)
        rng = np.random.default_rng(seed)
        self.sky = [O.pix2sky(wcs, band_pixels(self.shape, b, rng), O.WRAP_NONE) for b in self.bands]
        cuts = np.concatenate([[0], np.cumsum([len(s) for s in self.sky])])
        self.slices = [slice(int(cuts[k]), int(cuts[k + 1])) for k in range(len(self.bands))]
        self.all_sky = np.concatenate(self.sky)
        self._taps = {}
        for b in range(len(self.bands)):
            for order in (0, 1, 3):
                if order == 3 and min(self.shape) < 4:
                    continue
                idx = self.taps(O, b, order)
                tap_ref.window(idx, self.shape, self.bands[b].row0, self.bands[b].nrows, "raise", "%r, order %d" % (self.bands[b], order))
                assert (idx >= 0).any(), "%r: no tap of order %d on the map" % (self.bands[b], order)

    def taps(self, O, b, order):
        if (b, order) not in self._taps:
            self._taps[b, order] = order_taps(O, self.wcs, self.shape, self.sky[b], order)
        return self._taps[b, order]

    def offsets(self, O, b, plane, order):
        """(min, max) flat element offset of band b's taps of `order` in plane `plane` of the (nc, ny, nx) map."""
        idx = self.taps(O, b, order)
        on = idx[idx >= 0]
        base = plane * self.shape[0] * self.shape[1]
        return base + int(on.min()), base + int(on.max())

    def n_points(self):
        return len(self.all_sky)

    def band_elements(self):
        """Elements of one plane that lie in a band."""
        return sum(b.nrows for b in self.bands) * self.shape[0]


def tier_p(pj):
    """The 0.5 arcmin full sky, 43200 x 21601, periodic: plane offsets of maps of three and six planes."""
    shape, wcs = pj.fullsky_geometry(2 * math.pi / 43200)
    assert tuple(shape) == (43200, 21601)
    return (shape[0], shape[1]), wcs


def tier_r(pj):
    """Rows 1 .. 26000 of the 0.25 arcmin full sky, 86400 x 26000, periodic: 2.25e9 elements in ONE plane."""
    fshape, fwcs = pj.fullsky_geometry(2 * math.pi / 86400)
    shape, wcs = pj.slice_geometry(fshape, fwcs, None, (1, 26000))
    assert tuple(shape[:2]) == (86400, 26000)
    return (shape[0], shape[1]), wcs
