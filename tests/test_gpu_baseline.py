"""The two passes of the destriper on the device: pj.baseline_bin_pol_nearest and pj.baseline_project_pol_nearest
over pxl_baseline_{bin,project}_car_pol_nearest_f64, against the numpy yardstick tests/destripe_ref.py.

Maps: the 16 x 9 full sky (the seam is hit) and a 24 x 12 patch that is not periodic (points fall off it).  The points are
nearest_ref.points: over the map widened by 1.5 pixels, pixel edges and ties, far points, three positions that are not finite.

With small-integer d, a, w and map and dyadic responses every product and every sum is exact, so the order of the adds cannot
show: both passes must then give the yardstick's bits, chunk by chunk and accumulated over chunks.  With random Float64 inputs
the terms are still defined to the bit and only the order is free: bin is held to the scatters' clause (k - 1) 2^-53 sum|term|
per pixel of the exact sum, project to n 2^-52 sum|term| per baseline of the yardstick's math.fsum, and a second project call
must repeat the first bit for bit."""
import itertools
import math

import numpy as np
import pytest
import torch
from gpu_support import dev, to_dev

import destripe_ref as DR
import nearest_ref as N
from conftest import DEG, bits_equal

pytestmark = pytest.mark.gpu

# (D, T, baseline_len, chunk_t of the split run).  The project kernel gives a segment to a group of G lanes, G the power of two
# from 1 to 64 that covers baseline_len, and to a whole block of 256 from baseline_len 1024 on (two to four samples per lane and
# trip above 64 and 1024): 1, 7, 63, 64, 65, 130, 1000 and 1023 | 1024 take every G and both thresholds; 5000 is a segment longer
# than one block's trip of 1024 samples.  chunk_t never divides baseline_len, so later chunks start inside a baseline.
LAYOUTS = [(1, 1, 1, 1)] + [(3, 130, b, 47) for b in (1, 7, 63, 64, 65, 130, 1000)] + [(2, 1100, 1023, 401), (2, 1100, 1024, 401),
                                                                                      (1, 5000, 5000, 1733)]
GEOMS = ("cc_16x9", "box_24x12")
FORMS = ("d", "a", "da")


def _geom(pj, name):
    if name == "cc_16x9":
        g = pj.fullsky_geometry(2 * math.pi / 16)
    else:
        g = pj.geometry([[12 * DEG, -12 * DEG], [-6 * DEG, 6 * DEG]], 1.0 * DEG)
    assert tuple(g[0]) == {"cc_16x9": (16, 9), "box_24x12": (24, 12)}[name]
    return g


def _t(a, dev):
    return None if a is None else to_dev(a, dev)


class Obs:
    """One (D, T) observation on one map: sky, resp, w, d as (D, T, ...) arrays, the amplitudes a, a map m and a mask.  exact:
    everything a small integer or a dyadic fraction, so that no sum rounds.  The mask has zeros, a negative and a NaN pixel."""

    def __init__(self, pj, O, geom, nd, nt, blen, exact, seed):
        self.shape, self.wcs = _geom(pj, geom)
        nx, ny = self.shape
        self.nd, self.nt, self.blen, self.nb = nd, nt, blen, DR.n_base(nt, blen)
        rng = np.random.default_rng(seed)
        n = nd * nt
        self.sky = N.points(O, self.wcs, self.shape, n, seed).reshape(nd, nt, 2)
        if exact:
            self.resp = rng.integers(-4, 5, (nd, nt, 2)) / 4.0
            self.w = rng.integers(0, 5, (nd, nt)).astype(float)
            self.d = rng.integers(-8, 9, (nd, nt)).astype(float)
            self.a = rng.integers(-8, 9, nd * self.nb).astype(float)
            self.m = rng.integers(-32, 33, (3, ny, nx)) / 4.0
        else:
            psi = rng.uniform(0, np.pi, (nd, nt))
            self.resp = np.stack([np.cos(2 * psi), np.sin(2 * psi)], axis=-1) * rng.uniform(0.8, 1.0, (nd, nt, 1))
            self.w = 10.0 ** rng.uniform(-1, 1, (nd, nt))
            self.d = rng.normal(size=(nd, nt)) * 3
            self.a = rng.normal(size=nd * self.nb) * 5
            self.m = rng.normal(size=(3, ny, nx))
        self.mask = (rng.uniform(size=(ny, nx)) > 0.2).astype(float) * rng.integers(1, 4, (ny, nx))
        flat = self.mask.reshape(-1)
        flat[rng.integers(0, flat.size)] = -1.0
        flat[rng.integers(0, flat.size)] = np.nan

    def chunk(self, t0, nc):
        """The chunk's arrays, detector-major, as the kernels take them: (sky, resp, w, d)."""
        s = slice(t0, t0 + nc)
        return (self.sky[:, s].reshape(-1, 2), self.resp[:, s].reshape(-1, 2), self.w[:, s].reshape(-1), self.d[:, s].reshape(-1))

    def chunks(self, chunk_t):
        return [(t0, min(chunk_t, self.nt - t0)) for t0 in range(0, self.nt, chunk_t)]


def _calls(pj, O, dev, ob, t0, nc, form, with_m, with_mask, bin_out=None, proj_out=None):
    """Both passes on one chunk: ((device rhs, yardstick triple), (device baselines, yardstick quadruple))."""
    sky, resp, w, d = ob.chunk(t0, nc)
    d_ = d if "d" in form else None
    a_ = ob.a if "a" in form else None
    m_ = ob.m if with_m else None
    k_ = ob.mask if with_mask else None
    lay = (ob.nd, t0, ob.blen, ob.nb)
    dv = dict(d=_t(d_, dev), a=_t(a_, dev), mask=_t(k_, dev))
    args = (_t(w, dev), _t(sky, dev), _t(resp, dev), ob.shape, ob.wcs) + lay
    got_bin = pj.baseline_bin_pol_nearest(*args, out=_t(bin_out, dev), **dv).data.cpu().numpy()
    got_proj = pj.baseline_project_pol_nearest(*args, m=_t(m_, dev), out=_t(proj_out, dev), **dv)
    again = pj.baseline_project_pol_nearest(*args, m=_t(m_, dev), out=_t(proj_out, dev), **dv)
    assert bits_equal(got_proj.cpu().numpy(), again.cpu().numpy()), "project: a second call on the same arguments differs"
    ref_bin = DR.bin(O, ob.wcs, ob.shape, sky, resp, w, *lay, d=d_, a=a_, mask=k_, out=bin_out)
    ref_proj = DR.project(O, ob.wcs, ob.shape, sky, resp, w, *lay, d=d_, a=a_, m=m_, mask=k_, out=proj_out)
    return (got_bin, ref_bin), (got_proj.cpu().numpy(), ref_proj)


VARIANTS = [(f, m, k) for f, m, k in itertools.product(FORMS, (True, False), (True, False))]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "%dx%d_b%d" % l[:3])
@pytest.mark.parametrize("geom", GEOMS)
def test_exact_inputs_give_the_yardsticks_bits(pj, O, dev, geom, layout):
    """Small integers and dyadic responses: whole and split into chunks that start inside a baseline, every form of the sample
    value, with and without a map and a mask, both passes equal the yardstick bit for bit; bin also equals the device's own
    scatter_pol_nearest of the yardstick's products at the uncut samples.  Then the accumulation: rhs3 and out, started from
    integers, taken through all chunks, are the yardstick's bits too."""
    nd, nt, blen, chunk_t = layout
    ob = Obs(pj, O, geom, nd, nt, blen, True, 1000 + nt + blen)
    for ci, chunk_t_ in enumerate((nt, chunk_t)):
        for t0, nc in ob.chunks(chunk_t_):
            assert ci == 0 or t0 == 0 or blen == 1 or t0 % blen != 0
            for form, with_m, with_mask in VARIANTS:
                (gb, (rb, _k, _S)), (gp, (rp, _n, _S2, _tch)) = _calls(pj, O, dev, ob, t0, nc, form, with_m, with_mask)
                what = "%s, t0 = %d, n_chunk = %d, x = %s, map %s, mask %s" % (geom, t0, nc, form, with_m, with_mask)
                assert bits_equal(gb, rb), "bin: " + what
                assert bits_equal(gp, rp), "project: " + what
        # bin against the device's scatter of the yardstick's products, on the last chunk
        sky, resp, w, d = ob.chunk(t0, nc)
        v, live = DR.bin_products(DR.Chunk(O, ob.wcs, ob.shape, sky, w, nd, t0, blen, ob.nb, d=d, a=ob.a, mask=ob.mask))
        if live.any():
            sc = pj.scatter_pol_nearest(_t(v[live], dev), _t(sky[live], dev), _t(resp[live], dev), ob.shape, ob.wcs).data.cpu().numpy()
            assert bits_equal(_calls(pj, O, dev, ob, t0, nc, "da", True, True)[0][0], sc)
    rng = np.random.default_rng(7)
    acc_b = ref_b = rng.integers(-9, 10, (3, ob.shape[1], ob.shape[0])).astype(float)
    acc_p = ref_p = rng.integers(-9, 10, nd * ob.nb).astype(float)
    for t0, nc in ob.chunks(chunk_t):
        (acc_b, (ref_b, _k, _S)), (acc_p, (ref_p, _n, _S2, _tch)) = _calls(pj, O, dev, ob, t0, nc, "da", True, True, bin_out=ref_b, proj_out=ref_p)
        assert bits_equal(acc_b, ref_b) and bits_equal(acc_p, ref_p), "accumulated through t0 = %d" % t0


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: "%dx%d_b%d" % l[:3])
@pytest.mark.parametrize("geom", GEOMS)
def test_random_inputs_stay_within_the_rounding_bounds(pj, O, dev, geom, layout):
    nd, nt, blen, chunk_t = layout
    ob = Obs(pj, O, geom, nd, nt, blen, False, 2000 + nt + blen)
    worst_b = worst_p = 0.0
    for chunk_t_ in (nt, chunk_t):
        for t0, nc in ob.chunks(chunk_t_):
            for form, with_m, with_mask in VARIANTS:
                (gb, (rb, k, S)), (gp, (rp, n, S2, touched)) = _calls(pj, O, dev, ob, t0, nc, form, with_m, with_mask)
                what = "%s, t0 = %d, n_chunk = %d, x = %s, map %s, mask %s" % (geom, t0, nc, form, with_m, with_mask)
                eb, bb = np.abs(gb - rb), DR.bin_bound(rb, k, S)
                ep, bp = np.abs(gp - rp), DR.project_bound(n, S2)
                assert np.isfinite(gb).all() and np.isfinite(gp).all(), what
                assert np.all(eb <= bb), "bin: %s: worst excess %g" % (what, (eb - bb).max())
                assert np.all(ep <= bp), "project: %s: worst excess %g" % (what, (ep - bp).max())
                assert not gb[k == 0].view(np.int64).any() and not gp[~touched].view(np.int64).any(), what
                worst_b = max(worst_b, float((eb[bb > 0] / bb[bb > 0]).max()) if (bb > 0).any() else 0.0)
                worst_p = max(worst_p, float((ep[bp > 0] / bp[bp > 0]).max()) if (bp > 0).any() else 0.0)
    print("%s %s: worst error / bound: bin %.3g, project %.3g" % (geom, layout, worst_b, worst_p))


@pytest.mark.parametrize("blen", [1000, 100003])
def test_times_past_2_to_the_31(pj, O, dev, blen):
    """A chunk that starts past t0 = 2^31, 50 samples before a baseline's end: the kernels divide sample indices and times in 32
    bits only when every one of them fits 31, so this is the 64-bit form of both, which no small observation reaches.  Exact
    inputs, the yardstick's bits; the baselines before the chunk keep their value."""
    shape, wcs = _geom(pj, "box_24x12")
    nd, nc, t0 = 3, 130, (2 ** 31 // blen + 1) * blen - 50
    nb = (t0 + nc - 1) // blen + 1
    ob = Obs(pj, O, "box_24x12", nd, nc, blen, True, 3000 + blen)
    sky, resp, w, d = ob.chunk(0, nc)
    a = np.zeros(nd * nb)
    first = t0 // blen
    for det in range(nd):
        a[det * nb + first:det * nb + nb] = np.arange(1.0, nb - first + 1) + det
    lay = (nd, t0, blen, nb)
    args = (_t(w, dev), _t(sky, dev), _t(resp, dev), shape, wcs) + lay
    kw = dict(d=_t(d, dev), a=_t(a, dev), mask=_t(ob.mask, dev))
    init = np.full(nd * nb, 5.0)
    got_b = pj.baseline_bin_pol_nearest(*args, **kw).data.cpu().numpy()
    got_p = pj.baseline_project_pol_nearest(*args, m=_t(ob.m, dev), out=_t(init, dev), **kw).cpu().numpy()
    ref_b = DR.bin(O, wcs, shape, sky, resp, w, *lay, d=d, a=a, mask=ob.mask)[0]
    ref_p, n, _S, touched = DR.project(O, wcs, shape, sky, resp, w, *lay, d=d, a=a, m=ob.m, mask=ob.mask, out=init)
    assert t0 > 2 ** 31 and touched.sum() == 2 * nd and not touched.reshape(nd, nb)[:, :first].any()
    assert bits_equal(got_b, ref_b) and bits_equal(got_p, ref_p)


SENTINEL = np.array([0x7ff8dead0000beef], dtype=np.uint64).view(np.float64)[0]        # a NaN with a payload


def test_cut_samples_add_nothing(pj, O, dev):
    """On the patch: a NaN position, a point off the map and a point on a masked pixel each carry a NaN d and a NaN w, and add
    nothing to either output; the second detector's only baseline has nothing but such samples and keeps a NaN payload, -0.0
    and an ordinary value bit for bit; pixels and baselines that do get terms are exact."""
    shape, wcs = _geom(pj, "box_24x12")
    nx, ny = shape
    pix = np.array([[3.0, 2.0], [4.0, 2.0], [3.0, 2.0], [40.0, 2.0], [5.0, 5.0], [6.0, 6.0],         # detector 0: 3 and 4 and (NaN) 5 cut
                    [5.0, 5.0], [-2.0, 3.0], [7.0, 20.0], [5.0, 5.0], [5.0, 5.0], [1.0, 1.0]])       # detector 1: all cut
    sky = O.pix2sky(wcs, pix, O.WRAP_NONE)
    sky[5] = [np.nan, 0.1]
    sky[11] = [0.3, np.inf]
    mask = np.ones((ny, nx))
    mask[4, 4] = 0.0                                                                                  # pixel (5, 5)
    cut = np.array([0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1], bool)
    d = np.where(cut, np.nan, [1.0, 2.0, 3.0, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    w = np.where(cut, np.nan, 2.0)
    resp = np.tile([0.5, -0.25], (12, 1))
    m = np.zeros((3, ny, nx))
    m[:, 1, 2], m[:, 1, 3] = [1.0, 2.0, 4.0], [8.0, 0.0, 0.0]                                          # s = 1 + 1 - 1 = 1 and 8
    for blen, nb in ((6, 1), (4, 2)):
        for init in (SENTINEL, -0.0, 7.0):
            args = (_t(w, dev), _t(sky, dev), _t(resp, dev), shape, wcs, 2, 0, blen, nb)
            out = _t(np.full(2 * nb, init), dev)
            res = pj.baseline_project_pol_nearest(*args, d=_t(d, dev), m=_t(m, dev), mask=_t(mask, dev), out=out)
            assert res.data_ptr() == out.data_ptr()                          # out is accumulated into and returned
            got = res.cpu().numpy()
            keep = np.full(2 * nb, init)
            terms = 2.0 * (np.array([1.0, 2.0, 3.0]) - np.array([1.0, 8.0, 1.0]))       # baseline 0 holds the three uncut samples either way
            if not np.isnan(init):
                assert bits_equal(got[:1], np.array([init + terms.sum()]))
            assert bits_equal(got[1:], keep[1:]), "baselines without an uncut sample must keep their bits (%r)" % init
        rhs = pj.baseline_bin_pol_nearest(*args, d=_t(d, dev), mask=_t(mask, dev)).data.cpu().numpy()
        want = np.zeros((3, ny, nx))
        want[:, 1, 2] = [2.0 + 6.0, 0.5 * 8.0, -0.25 * 8.0]
        want[:, 1, 3] = [4.0, 2.0, -1.0]
        assert bits_equal(rhs, want)
        sent = np.full((3, ny, nx), SENTINEL)
        rhs = pj.baseline_bin_pol_nearest(*args, d=_t(d, dev), mask=_t(mask, dev), out=_t(sent, dev)).data.cpu().numpy()
        untouched = np.ones((ny, nx), bool)
        untouched[1, 2] = untouched[1, 3] = False
        assert bits_equal(rhs[:, untouched], sent[:, untouched])


def test_python_refusals(pj, O, dev):
    shape, wcs = _geom(pj, "cc_16x9")
    n = 12
    sky, resp, w, d = (_t(v, dev) for v in (np.full((n, 2), 0.1), np.zeros((n, 2)), np.ones(n), np.ones(n)))
    a = _t(np.zeros(6), dev)
    good = (w, sky, resp, shape, wcs, 3, 2, 4, 2)                                  # 3 detectors, times 2..5, baselines of 4: n_base 2
    for fn in (pj.baseline_bin_pol_nearest, pj.baseline_project_pol_nearest):
        fn(*good, d=d, a=a)
        with pytest.raises(ValueError, match="d, a or both"):
            fn(*good)
        with pytest.raises(ValueError, match="n_det"):
            fn(w, sky, resp, shape, wcs, 5, 2, 4, 2, d=d)
        with pytest.raises(ValueError, match="n_det >= 1"):
            fn(w, sky, resp, shape, wcs, 0, 2, 4, 2, d=d)
        with pytest.raises(ValueError, match="t0 >= 0"):
            fn(w, sky, resp, shape, wcs, 3, -1, 4, 2, d=d)
        with pytest.raises(ValueError, match="baseline_len >= 1"):
            fn(w, sky, resp, shape, wcs, 3, 2, 0, 2, d=d)
        with pytest.raises(ValueError, match="past n_base"):
            fn(w, sky, resp, shape, wcs, 3, 2, 4, 1, d=d)
        with pytest.raises(ValueError, match="amplitudes"):
            fn(*good, a=_t(np.zeros(5), dev))
        with pytest.raises(ValueError, match="mask is one"):
            fn(*good, d=d, mask=_t(np.ones((9, 15)), dev))
        with pytest.raises(ValueError, match="Float64 d"):
            fn(*good, d=d.float())
        with pytest.raises(ValueError, match="on one device"):
            fn(*good, d=_t(np.ones(n + 1), dev))
        with pytest.raises(RuntimeError, match="GPU"):
            fn(w.cpu(), sky, resp, shape, wcs, 3, 2, 4, 2, d=d)
        with pytest.raises(ValueError, match="CAR only"):
            fn(w, sky, resp, shape, pj.Gnomonic(wcs.cdelt, wcs.crpix, wcs.crval), 3, 2, 4, 2, d=d)
    with pytest.raises(ValueError, match="overlap"):
        pj.baseline_project_pol_nearest(*good, d=d, a=a, out=a)
    buf = torch.ones((4, 9, 16), dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="overlap"):
        pj.baseline_bin_pol_nearest(*good, d=d, mask=buf[2], out=buf[:3])
    with pytest.raises(ValueError, match="IQU map"):
        pj.baseline_project_pol_nearest(*good, d=d, m=torch.zeros((2, 9, 16), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="amplitudes"):
        pj.baseline_project_pol_nearest(*good, d=d, out=torch.zeros(7, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="map on"):
        pj.baseline_bin_pol_nearest(*good, d=d, out=torch.zeros((3, 9, 15), dtype=torch.float64, device=dev))
