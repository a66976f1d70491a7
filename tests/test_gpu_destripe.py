"""pj.destripe_map_pol_nearest_tod on the device against the dense yardstick tests/destripe_ref.py, on its
end-to-end case: four detectors raster a 12 x 7 patch along RA and then along DEC, 600 samples each, with random polarisation
angles; offsets of rms 5 per baseline of 37 samples are added to noiseless samples of a random sky.

The yardstick runs on the device's own expanded pointing (the same inputs), with the same tol and maxiter and the package's own
pcg.  Maps are compared after the mean of I over the solved pixels is removed from both: the gauge.  The device's error against
the true sky may be at most 10 x the yardstick's: atomic ordering perturbs each A p in the last bits and CG amplifies that by the
operator's condition number, a few tens here."""
import numpy as np
import pytest
import torch
from gpu_support import dev, to_dev

import destripe_ref as DR
import scatter_ref as R

pytestmark = pytest.mark.gpu


class Case:
    """The scan on the device: quaternions, the device's expansion of them brought back for the yardstick, the timestream with
    offsets, and the yardstick's destriped map of it.  nan_times: boresight samples whose quaternion is NaN."""

    def __init__(self, pj, O, dev, nan_times=None):
        self.scan = s = DR.Scan(pj)
        qb, qd = s.quaternions(pj, O)
        if nan_times is not None:
            qb[nan_times] = float("nan")
        self.q_bore, self.q_det = qb.to(dev), qd.to(dev)
        sky, resp = pj.expand_pointing(self.q_bore, self.q_det)
        self.sky, self.resp = sky.cpu().numpy(), resp.cpu().numpy()
        self.w = to_dev(s.w_det, dev)
        self.dense = s.dense(O, self.sky, self.resp)
        self.tod_np = s.tod(O, self.sky, self.resp)                        # NaN where the quaternion is: a cut sample's d is NaN
        self.tod = to_dev(self.tod_np, dev)
        self.ref_map, self.ref_a, self.ref_info = self.dense.destripe(pj, self.tod_np, s.TOL, s.MAXITER)
        self.ref_err = DR.map_error(self.ref_map, s.m0, self.dense.solved)

    def run(self, pj, tod=None, **kw):
        s = self.scan
        return pj.destripe_map_pol_nearest_tod(self.tod if tod is None else tod, self.w, self.q_bore, self.q_det, None, s.shape, s.wcs,
                                               s.BLEN, rcond_min=s.RCOND_MIN, tol=s.TOL, maxiter=s.MAXITER, **kw)


@pytest.fixture(scope="module")
def case(pj, O, dev):
    return Case(pj, O, dev)


def test_it_recovers_the_sky_where_the_binned_map_is_striped(pj, dev, case):
    s = case.scan
    m, rcond, weights, a, info = case.run(pj)
    nx, ny = s.shape
    assert tuple(m.data.shape) == (3, ny, nx) and tuple(rcond.data.shape) == (ny, nx) and tuple(weights.data.shape) == (6, ny, nx)
    assert tuple(a.shape) == (s.ND, s.nb)
    assert info["converged"] and not info["breakdown"]
    solved = rcond.data.cpu().numpy() >= s.RCOND_MIN
    assert solved.all() and np.array_equal(solved, case.dense.solved)
    err = DR.map_error(m.data.cpu().numpy(), s.m0, solved)
    mb = pj.binned_map_pol_nearest_tod(case.tod, case.w, case.q_bore, case.q_det, None, s.shape, s.wcs, rcond_min=s.RCOND_MIN)[0]
    binned = DR.map_error(mb.data.cpu().numpy(), s.m0, solved)
    an = a.cpu().numpy()
    da = np.abs((an - an.mean()) - (s.a0 - s.a0.mean())).max()
    print("device: %d iterations, map error %.3g; yardstick: %d iterations, map error %.3g; ratio %.3g; binned map error %.3g; "
          "baselines off by %.3g" % (info["iterations"], err, case.ref_info["iterations"], case.ref_err, err / case.ref_err, binned, da))
    assert err <= 10 * case.ref_err
    assert binned > 1000 * case.ref_err
    assert da <= 10 * np.abs((case.ref_a - case.ref_a.mean()) - (s.a0 - s.a0.mean())).max()


@pytest.mark.parametrize("chunk_t", [37, 100, 251, 599])
def test_chunks_that_cut_baselines(pj, O, dev, case, chunk_t):
    """chunk_t = 100, 251 and 599 start chunks inside baselines of 37 samples, 37 itself puts every baseline in a chunk of its
    own.  With the baselines held fixed, the two passes taken through the map-maker's own chunks agree with one whole-observation
    call to the rounding of their sums: the binned rhs to the scatters' clause k 2^-52 S per pixel (two atomic accumulations of
    the same terms), the projection to (n + 1) 2^-52 S per baseline (two fixed orders of the same n terms, (n - 1) 2^-53 S each at most, and one
    rounding more, 2^-53 S, for each of the at most two chunks a baseline meets here).
    The map-maker itself is held to what the unchunked run is held to."""
    from pixell_jl_amd import mapmaker
    s = case.scan
    a = to_dev(s.a0.reshape(-1), dev)
    m0 = to_dev(s.m0, dev)
    sky, resp = to_dev(case.sky, dev), to_dev(case.resp, dev)
    w_all = case.w[:, None].expand(s.ND, s.NT).reshape(-1).contiguous()
    lay = (s.shape, s.wcs, s.ND, 0, s.BLEN, s.nb)
    whole_b = pj.baseline_bin_pol_nearest(w_all, sky, resp, *lay, d=case.tod.reshape(-1), a=a).data.cpu().numpy()
    whole_p = pj.baseline_project_pol_nearest(w_all, sky, resp, *lay, d=case.tod.reshape(-1), a=a, m=m0).cpu().numpy()
    rhs, out = None, None
    src = mapmaker._TodChunks("test", case.tod, case.w, case.q_bore, case.q_det, None, chunk_t)
    for i, (d, wc, sk, rs) in enumerate(src.chunks()):
        lay_c = (s.shape, s.wcs, s.ND, i * chunk_t, s.BLEN, s.nb)
        rhs = pj.baseline_bin_pol_nearest(wc, sk, rs, *lay_c, d=d, a=a, out=rhs)
        out = pj.baseline_project_pol_nearest(wc, sk, rs, *lay_c, d=d, a=a, m=m0, out=out)
    _ref, k, S = DR.bin(O, s.wcs, s.shape, case.sky, case.resp, w_all.cpu().numpy(), s.ND, 0, s.BLEN, s.nb,
                        d=case.tod_np.reshape(-1), a=s.a0.reshape(-1))
    R.held(rhs.data.cpu().numpy(), whole_b, k, S, "rhs, chunk_t = %d against whole" % chunk_t)
    _r, nterm, S2, _tch = DR.project(O, s.wcs, s.shape, case.sky, case.resp, w_all.cpu().numpy(), s.ND, 0, s.BLEN, s.nb,
                                     d=case.tod_np.reshape(-1), a=s.a0.reshape(-1), m=s.m0)
    assert np.all(np.abs(out.cpu().numpy() - whole_p) <= (nterm + 1) * 2.0 ** -52 * S2)
    m, rcond, _wts, _a, info = case.run(pj, chunk_t=chunk_t)
    err = DR.map_error(m.data.cpu().numpy(), s.m0, rcond.data.cpu().numpy() >= s.RCOND_MIN)
    print("chunk_t = %d: %d iterations, map error %.3g (yardstick %.3g)" % (chunk_t, info["iterations"], err, case.ref_err))
    assert info["converged"] and err <= 10 * case.ref_err


def test_no_offsets(pj, O, dev, case):
    """A timestream of zeros has a right-hand side of exactly zero: pcg stops at rz0 == 0, the baselines are +0.0 and the map is
    the binned map, bit for bit.  Noiseless samples without offsets leave a right-hand side of rounding alone, whose solution is
    one constant (the gauge) plus rounding: apart from that constant the baselines and the map are held to 1e-5, the bound of
    tests/test_destripe_ref.py for the case with offsets, which carries more."""
    s = case.scan
    zero = torch.zeros_like(case.tod)
    m, _rc, _wts, a, info = case.run(pj, tod=zero)
    mb = pj.binned_map_pol_nearest_tod(zero, case.w, case.q_bore, case.q_det, None, s.shape, s.wcs, rcond_min=s.RCOND_MIN)[0]
    assert info["iterations"] == 0 and info["converged"]
    assert not a.cpu().numpy().view(np.int64).any()
    assert np.array_equal(m.data.cpu().numpy().view(np.int64), mb.data.cpu().numpy().view(np.int64))
    clean = to_dev(s.tod(O, case.sky, case.resp, offsets=False), dev)
    m, rc, _wts, a, info = case.run(pj, tod=clean)
    mb = pj.binned_map_pol_nearest_tod(clean, case.w, case.q_bore, case.q_det, None, s.shape, s.wcs, rcond_min=s.RCOND_MIN)[0]
    solved = rc.data.cpu().numpy() >= s.RCOND_MIN
    an = a.cpu().numpy()
    gap = DR.map_error(m.data.cpu().numpy(), mb.data.cpu().numpy(), solved)
    print("no offsets: %d iterations, baselines mean %.3g spread %.3g, destriped against binned %.3g" % (info["iterations"], an.mean(), np.abs(an - an.mean()).max(), gap))
    assert np.abs(an - an.mean()).max() <= 1e-5 and gap <= 1e-5


def test_cut_samples_do_not_raise(pj, O, dev):
    """NaN boresight quaternions while the boresight is over columns 4 to 6, rows 2 to 5 of the patch: the samples are cut, the
    pixels at the heart of that region get no hits, are unsolved and masked, and the samples other detectors and times put on
    them are cut too.  Nothing raises; unsolved pixels are +0.0; the solved ones are held to 10 x the yardstick, which is given
    the same NaN positions; a baseline with no uncut sample is +0.0."""
    scan = DR.Scan(pj)
    hole = (scan.pix[:, 0] > 3.5) & (scan.pix[:, 0] < 6.5) & (scan.pix[:, 1] > 1.5) & (scan.pix[:, 1] < 5.5)
    c = Case(pj, O, dev, nan_times=torch.from_numpy(hole))
    s = c.scan
    m, rcond, _wts, a, info = c.run(pj)
    solved = rcond.data.cpu().numpy() >= s.RCOND_MIN
    mm = m.data.cpu().numpy()
    print("%d boresight samples NaN, %d pixels unsolved, %d samples cut; device error %.3g, yardstick %.3g"
          % (hole.sum(), (~solved).sum(), (~c.dense.live).sum(), DR.map_error(mm, s.m0, solved), c.ref_err))
    assert hole.sum() > 20 and (~solved).sum() >= 1 and np.array_equal(solved, c.dense.solved)
    assert info["converged"] and np.isfinite(mm).all() and np.isfinite(a.cpu().numpy()).all()
    assert not mm[:, ~solved].view(np.int64).any()
    assert DR.map_error(mm, s.m0, solved) <= 10 * c.ref_err
    empty = np.bincount(c.dense.b[c.dense.live], minlength=s.ND * s.nb) == 0
    assert not a.cpu().numpy().reshape(-1)[empty].view(np.int64).any()
