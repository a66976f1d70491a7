"""The polarised map-makers: five public functions over one accumulate-and-solve path, and the destriper.

pcg() is preconditioned conjugate gradients alone, on torch tensors of any device: it calls nothing of the library, only the two
operators it is given.

A map-maker is {a source of samples} x {pointing order, fused or composed} x {one block solve, or CG}:

    source      _Batches: a list of (d, w, skycoords, resp).  _TodChunks: the time chunks of a (D, T) observation, expanded from
                quaternion pointing one chunk at a time.  Either can be passed over any number of times: source.chunks() yields
                (d, w, skycoords, resp) in order.
    _accumulate rhs = P^T W d and the six weight planes of one pass over a source.
    _binned     one pol_block_solve of them in place: binned_map_pol (order 1, one batch), binned_map_pol_nearest (order 0; DESIGN
                4.15: there P^T W P is exactly its pixel blocks, so this is the least-squares map) and binned_map_pol_nearest_tod.
    _cg         block-Jacobi PCG on P^T W P m = P^T W d, one pass over the source per application of the normal operator:
                cg_map_pol and cg_map_pol_tod.
    destriper   destripe_map_pol_nearest_tod: one offset per detector and baseline solved by pcg with the sky projected
                out, over _TodChunks at order 0; it stands beside the five and shares only the source and _accumulate with them.
    filter-bin  filter_bin_map_pol_nearest_tod: a polynomial per detector and scan fitted off the masked sky and
                subtracted (ops.polyfilter_tod), then _binned at order 0 over the same _TodChunks with the filtered timestream.
                With modes= the detector modes of DESIGN 4.19 are fitted and subtracted per time sample after it (ops.modefilter_tod),
                template_bin_map_pol_nearest_tod is the same path with the binned templates per detector and bin
                between the two (ops.binfilter_tod).
    ML          ml_map_pol_nearest_tod: the maximum-likelihood map under stationary correlated noise, pcg on
                (P^T N^-1 P) m = P^T N^-1 d with N^-1 the banded-Toeplitz weight of ops.toeplitz_tod applied to the whole (D, T)
                array between a sampling and a scattering pass over _TodChunks at order 0; the white-noise pixel blocks are its
                preconditioner.

Every operator is looked up in ops at call time.  The public functions hold their own argument checks, in their own order, and
say where they differ."""
import math

import torch

from . import ops
from .enmap import Enmap


def _dot(a: torch.Tensor, b: torch.Tensor) -> float:
    return float(torch.dot(a.reshape(-1), b.reshape(-1)))


def pcg(apply_a, apply_minv, b: torch.Tensor, tol, maxiter):
    """Preconditioned conjugate gradients for A x = b, A symmetric positive definite: apply_a(p) returns A p, apply_minv(r) returns
    M^-1 r (M symmetric positive definite), both as new tensors of b's shape; b is a Float64 tensor of any shape and device.
    Returns (x, info), info = {"iterations", "converged", "breakdown", "history"}.

        x = 0, r = b, z = M^-1 r, p = z, rz = <r, z>, rz0 = rz
        rz0 == 0: return zeros, converged, 0 iterations;  rz0 NaN, Inf or negative: ValueError
        each iteration:  q = A p, pq = <p, q>;  pq not finite or not > 0: stop, info["breakdown"] = True
                         alpha = rz / pq, x += alpha p, r -= alpha q, z = M^-1 r, rz' = <r, z>
                         history.append(sqrt(rz' / rz0));  rz' <= tol^2 rz0: stop, converged
                         p = z + (rz' / rz) p, rz = rz'

    The stopping norm is the M^-1 norm of the recursive residual relative to its start, sqrt(<r, M^-1 r> / <b, M^-1 b>).
    "iterations" counts completed updates of x.  An rz' that is NaN or negative (an M^-1 that is not positive definite) also
    stops with breakdown.  Dot products are Float64 torch.dot on the flattened tensors, read back to the host: two scalars per
    iteration, negligible beside a map-sized operator.  Non-finite right-hand sides are refused, not iterated on."""
    if not isinstance(b, torch.Tensor) or b.dtype != torch.float64:
        raise TypeError("pcg works on Float64 torch tensors")
    tol, maxiter = float(tol), int(maxiter)
    if not (tol > 0.0) or maxiter < 0:
        raise ValueError("pcg needs tol > 0 and maxiter >= 0")
    x = torch.zeros_like(b)
    r = b.clone()
    z = apply_minv(r)
    p = z.clone()
    rz = rz0 = _dot(r, z)
    info = {"iterations": 0, "converged": False, "breakdown": False, "history": []}
    if rz0 == 0.0:
        info["converged"] = True
        return x, info
    if not math.isfinite(rz0) or rz0 < 0.0:
        raise ValueError("pcg: <b, M^-1 b> = %r: the right-hand side is not finite, or M^-1 is not positive definite "
                         "(cut non-finite samples with w = 0 before they reach the map)" % rz0)
    for _ in range(maxiter):
        q = apply_a(p)
        pq = _dot(p, q)
        if not (math.isfinite(pq) and pq > 0.0):
            info["breakdown"] = True
            break
        alpha = rz / pq
        x.add_(p, alpha=alpha)
        r.sub_(q, alpha=alpha)
        z = apply_minv(r)
        rz_new = _dot(r, z)
        info["iterations"] += 1
        if not (math.isfinite(rz_new) and rz_new >= 0.0):
            info["history"].append(float("nan"))
            info["breakdown"] = True
            break
        info["history"].append(math.sqrt(rz_new / rz0))
        if rz_new <= tol * tol * rz0:
            info["converged"] = True
            break
        p = z.add(p, alpha=rz_new / rz)
        rz = rz_new
    return x, info


# ---- the sources of samples ---------------------------------------------------------------------------------------------------
# A source is passed over with source.chunks(with_d=True), which yields (d, w, skycoords, resp) in order: (N,) samples and
# weights, (N, 2) coordinates and responses on one device.  A consumer is done with a tuple (on the current stream) before it
# asks for the next.  with_d=False is for a consumer that does not read d (the normal operator); d may then be None.

class _Batches:
    """The source that is a list of batches.  Built from any iterable, which it consumes once; at least one batch."""

    def __init__(self, what, batches):
        self.what, self.batches = what, list(batches)
        if not self.batches:
            raise ValueError("%s needs at least one batch (d, w, skycoords, resp)" % what)

    def checked(self, no_f32=False):
        """The batch checks of the caller `what`: four items, ops._sample_vectors on d and w, and with no_f32 the caller's own
        refusal of Float32 for all four (without it skycoords and resp are left to the scatters)."""
        for bt in self.batches:
            if len(bt) != 4:
                raise ValueError("a batch is (d, w, skycoords, resp)")
            if no_f32:
                for t, noun in zip(bt, ("d", "w", "skycoords", "resp")):
                    ops._no_f32(self.what, t, noun)
            ops._sample_vectors(self.what, bt[0], bt[1])
        return self

    def chunks(self, with_d=True):
        return iter(self.batches)


class _TodChunks:
    """The source that is a (D, T) observation with quaternion pointing, in time chunks [t0, t0 + chunk_t),
    detector-major as expand_pointing writes them.  tod is (D, T); w is (D, T) or (D,); q_bore (T, 4), q_det (D, 4) and gamma
    ((D,) or None) are expand_pointing's, which checks their values itself on the first chunk.  chunk_t=None is
    max(1, min(T, 2^24 // D)); any chunk_t is clamped to T.

    Every pass expands one chunk at a time into the source's two (D * chunk_t, 2) buffers: skycoords and resp are views of
    them that the next chunk overwrites, so the chunks of a pass cannot be kept (no list() of them), and the 32 B per sample of
    expanded pointing never exist for the whole observation.  d and w are the chunk's samples and weights made contiguous
    (copies, unless the chunk is the whole observation); with_d=False skips the copy of d, 8 B per sample.  Peak extra memory:
    32 * D * chunk_t bytes of pointing plus 16 * D * chunk_t of d and w."""

    def __init__(self, what, tod, w, q_bore, q_det, gamma, chunk_t):
        for t, noun in ((tod, "tod"), (w, "w")):
            ops._no_f32(what, t, noun)
            ops._dev_f64(t, noun)
        if tod.dim() != 2 or tod.shape[0] < 1 or tod.shape[1] < 1:
            raise ValueError("%s: tod is a (D, T) tensor with at least one sample" % what)
        nd, nt = tod.shape
        if tuple(w.shape) not in ((nd, nt), (nd,)) or w.device != tod.device:
            raise ValueError("%s: w is (D, T) or (D,) on the device of tod" % what)
        for t, noun, rows in ((q_bore, "q_bore", nt), (q_det, "q_det", nd)):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or tuple(t.shape) != (rows, 4):
                raise ValueError("%s: %s is (%d, 4) for this tod" % (what, noun, rows))
        if chunk_t is None:
            chunk_t = max(1, min(nt, (1 << 24) // nd))            # 2^24 samples: 512 MiB of expanded pointing
        chunk_t = int(chunk_t)
        if chunk_t < 1:
            raise ValueError("%s: chunk_t must be at least 1" % what)
        self.chunk_t = min(chunk_t, nt)
        self.tod, self.w, self.pointing = tod, w, (q_bore, q_det, gamma)
        self.sky_buf = torch.empty((nd * self.chunk_t, 2), dtype=torch.float64, device=tod.device)
        self.resp_buf = torch.empty_like(self.sky_buf)

    def chunks(self, with_d=True):
        tod, w, (q_bore, q_det, gamma) = self.tod, self.w, self.pointing
        nd, nt = tod.shape
        for t0 in range(0, nt, self.chunk_t):
            ct = min(self.chunk_t, nt - t0)
            sky, resp = ops.expand_pointing(q_bore[t0:t0 + ct], q_det, gamma, out_sky=self.sky_buf[:nd * ct], out_resp=self.resp_buf[:nd * ct])
            d = tod[:, t0:t0 + ct].reshape(-1).contiguous() if with_d else None      # (a one-sample chunk reshapes to a strided view)
            wc = (w[:, t0:t0 + ct] if w.dim() == 2 else w[:, None].expand(nd, ct)).reshape(-1).contiguous()
            yield d, wc, sky, resp


# ---- one accumulation, one solve for the binned maps, one CG driver -----------------------------------------------------------

def _accumulate(what, source, shape, wcs, order, fused=True, check_finite=True):
    """(rhs, weights) of one pass over `source`: rhs = P^T W d, (3, ny, nx), and the six planes II, IQ, IU, QQ, QU, UU of
    P^T W P's pixel blocks, (6, ny, nx), for the pointing matrix of `order`.  Order 0 takes one bin_pol_nearest per tuple, or with
    fused=False scatter_pol_nearest(w * d) and scatter_pol_weights_nearest(w): the same terms bit for bit.  Order 1 takes
    scatter_pol(w * d) and scatter_pol_weights(w).  The first tuple's calls allocate, the others accumulate through out=.

    check_finite: a NaN or Inf in rhs raises ValueError in the name of `what` -- non-finite samples are the caller's to cut, with
    w = 0 AND a finite d (0 * NaN is NaN).  That read of one flag is the pass's only host synchronisation."""
    rhs = weights = None
    for d, w, sky, resp in source.chunks():
        if order == 0 and fused:
            rhs, weights = ops.bin_pol_nearest(d, w, sky, resp, shape, wcs, rhs=rhs, weights=weights)
        elif order == 0:
            rhs = ops.scatter_pol_nearest(w * d, sky, resp, shape, wcs, out=rhs)
            weights = ops.scatter_pol_weights_nearest(w, sky, resp, shape, wcs, out=weights)
        else:
            rhs = ops.scatter_pol(w * d, sky, resp, shape, wcs, order=1, out=rhs)
            weights = ops.scatter_pol_weights(w, sky, resp, shape, wcs, order=1, out=weights)
    if check_finite and not bool(torch.isfinite(rhs.data).all()):
        raise ValueError("%s: P^T W d is not finite: cut non-finite samples with w = 0 and a finite d" % what)
    return rhs, weights


def _binned(what, source, shape, wcs, rmin, order, fused=True, check_finite=True):
    """(map, rcond, weights): _accumulate, then pol_block_solve in place in rhs.  Unsolved pixels (pol_block_solve's rule: no
    hits, fewer than three, one polarisation angle, a pivot ratio below rmin) are +0.0 in the map; cut on rcond."""
    rhs, weights = _accumulate(what, source, shape, wcs, order, fused, check_finite)
    m, rcond = ops.pol_block_solve(rhs, weights, rcond_min=rmin, out=rhs, return_rcond=True)
    return m, rcond, weights


def _cg(what, source, shape, wcs, rmin, tol, maxiter, fused=True):
    """(map, rcond, info): _accumulate at order 1, rcond from one pol_block_solve, then pcg with M^-1 = pol_block_solve(.,
    weights, rmin) and A p = the sum over one pass of the source of normal_pol(p, w, skycoords, resp), accumulated into a zeroed
    map -- with fused=False of scatter_pol(w * sample_pol(p)) instead: the same terms bit for bit, three launches and an
    N-length temporary per tuple.  tol and maxiter are pcg's, which checks them: after the accumulation."""
    rhs, weights = _accumulate(what, source, shape, wcs, 1)
    _z, rcond = ops.pol_block_solve(rhs, weights, rcond_min=rmin, return_rcond=True)

    def apply_a(p):
        y = torch.zeros_like(p)
        pm = Enmap(p, wcs)
        for _d, w, sky, resp in source.chunks(with_d=False):
            if fused:
                ops.normal_pol(pm, w, sky, resp, out=y)
            else:
                ops.scatter_pol(w * ops.sample_pol(pm, sky, resp), sky, resp, shape, wcs, out=y)
        return y

    def apply_minv(r):
        return ops.pol_block_solve(Enmap(r, wcs), weights, rcond_min=rmin).data

    x, info = pcg(apply_a, apply_minv, rhs.data, tol, maxiter)
    return Enmap(x, wcs), rcond, info


# ---- the five map-makers --------------------------------------------------------------------------------------------------------
# Their checks differ, and nothing here unifies them.  The order-1 batch forms leave the CAR-only and Float32 refusals of
# skycoords and resp to scatter_pol; the order-0 and _tod forms make them in their own name.  binned_map_pol checks its one batch
# before rcond_min, the list forms after; it alone does not check rhs for finiteness, and so never waits for the device.

def binned_map_pol(d: torch.Tensor, w: torch.Tensor, skycoords: torch.Tensor, resp: torch.Tensor, shape, wcs, rcond_min=1e-3):
    """The binned polarised map (P^T W P restricted to its pixel blocks)^-1 P^T W d of the (N,) samples `d` with the (N,) weights
    `w` at a 2xN batch of (ra, dec) with responses `resp` (as for scatter_pol): _binned at order 1 of that one batch.  Returns
    (map, rcond): the (3, ny, nx) IQU Enmap, unsolved pixels +0.0, and the (ny, nx) conditioning Enmap to cut on.  A non-finite
    sample is not refused: it makes its pixels unsolved, and the call returns without a device-to-host read.

    Order 1 only.  At order 3 the pointing matrix is E F and the transposed prefilter F^T has negative entries, so the
    prefiltered weight planes are not sums of w p p^T: the pixel blocks are no longer positive semi-definite, and neither the
    pivoting nor the conditioning above means anything on them.

    Many batches: accumulate both scatters with out=, then solve once,

        rhs = pj.scatter_pol(w0 * d0, sky0, resp0, shape, wcs)
        wts = pj.scatter_pol_weights(w0, sky0, resp0, shape, wcs)
        for d, w, sky, resp in batches:
            pj.scatter_pol(w * d, sky, resp, shape, wcs, out=rhs)
            pj.scatter_pol_weights(w, sky, resp, shape, wcs, out=wts)
        m, rcond = pj.pol_block_solve(rhs, wts, out=rhs, return_rcond=True)
    """
    source = _Batches("binned_map_pol", [(d, w, skycoords, resp)]).checked()
    rmin = ops._rcond_min(rcond_min)
    return _binned("binned_map_pol", source, shape, wcs, rmin, 1, check_finite=False)[:2]


def cg_map_pol(batches, shape, wcs, rcond_min=1e-3, tol=1e-8, maxiter=200, fused=True):
    """The least-squares polarised map: the m that minimises |W^(1/2) (d - P m)|, P the order-1 pointing matrix of sample_pol and
    W diagonal, by block-Jacobi-preconditioned CG on P^T W P m = P^T W d: _cg over the list of `batches`, each
    (d, w, skycoords, resp): (N,) samples and weights, (N, 2) coordinates and responses, as for binned_map_pol.  Returns
    (map, rcond, info): the (3, ny, nx) IQU Enmap, the (ny, nx) conditioning Enmap of the pixel blocks, and pcg's info.

    fused=False forms A p by the composition _cg names.  On the MI355X (10^8 points on a 43200 x 21601 x 3 map) the fused call
    was 1.30-1.35x faster than that composition on sphere-uniform points and level with it (1.02x) on raster-ordered ones
    (DESIGN 4.14).

    Unsolved pixels (pol_block_solve's rule: no hits, fewer than three, one polarisation angle, a pivot ratio below
    rcond_min) get z = +0.0 from M^-1, so p and x stay exactly +0.0 there in all three planes: the iteration is PCG on the
    principal sub-system of the solved pixels, and what the samples say about the other pixels is left in the residual.
    binned_map_pol is NOT this map: with bilinear pointing P^T W P couples neighbouring pixels and the binned map inverts only
    the pixel blocks (it is the first z of this iteration).

    rcond_min bounds the condition of each pixel block, not cond(P^T W P), and the iteration count follows the latter.  With
    at least ~50 points per pixel, uniform in pixel space, cond of the preconditioned system was 10-20 and tol = 1e-8 took 10-36
    iterations.  With 10^6 points uniform on the SPHERE on a 360 x 181 map the pixels near the pole rows are thinly hit:
    rcond_min = 1e-3 accepted 96.8 % of the pixels and PCG was still at a relative residual of 1.2e-4 after 2000 iterations,
    with |x| up to 1e4; rcond_min = 0.1 took 607 iterations.  Cut on the returned rcond and watch info: "converged" False or
    "breakdown" True means the map is not the solution.

    A NaN or Inf that reaches rhs raises ValueError (_accumulate).  Order 1 only, for binned_map_pol's reason; Float64, CAR, one
    device."""
    source = _Batches("cg_map_pol", batches)
    rmin = ops._rcond_min(rcond_min)
    return _cg("cg_map_pol", source.checked(), shape, wcs, rmin, tol, maxiter, fused)


def binned_map_pol_nearest(batches, shape, wcs, rcond_min=1e-3, fused=True):
    """The polarised map of nearest-pixel (order 0) pointing: one pass over the samples and one per-pixel solve, no
    iteration: _binned at order 0 over the list of `batches`, each (d, w, skycoords, resp) as for cg_map_pol.  Returns
    (map, rcond, weights): the (3, ny, nx) IQU Enmap, the (ny, nx) conditioning Enmap of the pixel blocks, and the (6, ny, nx)
    Enmap of the weight planes II, IQ, IU, QQ, QU, UU.

    fused=False accumulates by the composition _accumulate names: two launches, a torch multiply and an N-length temporary per
    batch.  On the MI355X (10^8 points on a 43200 x 21601 x 3 map) the fused call took 43.7 ms on sphere-uniform points and
    24.6 ms on raster-ordered ones against 44.2 and 25.2 ms for that composition: level, the nine atomics per point being all of
    either form's time.

    With nearest-pixel pointing every sample touches one pixel, so P^T W P has no entries outside the per-pixel 3 x 3 blocks:
    `weights` is EXACTLY P^T W P, which for white noise of variance 1 / w is the inverse covariance of the map, and this map
    IS the least-squares map for this P -- the m that minimises |W^(1/2) (d - P m)| on the solved pixels -- where the order-1
    binned_map_pol only inverts the diagonal blocks of a coupled system.  That is why order 0 has no CG map-maker and no
    normal-operator kernel: pol_block_apply(x, weights) is P^T W P x.

    A NaN or Inf that reaches rhs raises ValueError (_accumulate).  Float64, CAR, full maps, one device."""
    what = "binned_map_pol_nearest"
    source = _Batches(what, batches)
    ops._car_only(wcs, what)
    rmin = ops._rcond_min(rcond_min)
    return _binned(what, source.checked(no_f32=True), shape, wcs, rmin, 0, fused)


def binned_map_pol_nearest_tod(tod, w, q_bore, q_det, gamma, shape, wcs, rcond_min=1e-3, chunk_t=None):
    """binned_map_pol_nearest from time-ordered data and quaternion pointing: _binned at order 0, fused, over
    _TodChunks, whose arguments, chunking and peak memory are described there.  tod: the (D, T) samples of D detectors; w: their
    weights, (D, T) or one per detector (D,); q_bore (T, 4), q_det (D, 4), gamma ((D,) or None): the arguments of
    expand_pointing; chunk_t: samples per detector and chunk (None: 2^24 // D).  Returns (map, rcond, weights) as
    binned_map_pol_nearest does, and raises what it raises.  A boresight or detector quaternion that is NaN, Inf or all zeros
    cuts its samples (their position is NaN and bin_pol_nearest adds nothing for them).  The accumulation order of the atomics
    differs from the batch form's, so the two maps agree to the scatters' rounding clause, not to the bit."""
    what = "binned_map_pol_nearest_tod"
    ops._car_only(wcs, what)
    rmin = ops._rcond_min(rcond_min)
    return _binned(what, _TodChunks(what, tod, w, q_bore, q_det, gamma, chunk_t), shape, wcs, rmin, 0)


def cg_map_pol_tod(tod, w, q_bore, q_det, gamma, shape, wcs, rcond_min=1e-3, tol=1e-8, maxiter=200, chunk_t=None):
    """cg_map_pol (order 1, fused) from time-ordered data and quaternion pointing: _cg over _TodChunks; arguments
    as for binned_map_pol_nearest_tod, tol and maxiter as for cg_map_pol.  Every application of the normal operator is a pass
    over the source, which expands each chunk again (without the copy of d), so the expansion kernel runs (iterations + 2) times
    over the observation and nothing of size D * T is ever held besides tod and w.  Returns (map, rcond, info) as cg_map_pol
    does, and raises what it raises."""
    what = "cg_map_pol_tod"
    ops._car_only(wcs, what)
    rmin = ops._rcond_min(rcond_min)
    return _cg(what, _TodChunks(what, tod, w, q_bore, q_det, gamma, chunk_t), shape, wcs, rmin, tol, maxiter)


# ---- the filter-and-bin map -----------------------------------------------------------------------------------------

def filter_bin_map_pol_nearest_tod(tod, w, q_bore, q_det, gamma, shape, wcs, seg_start, order, fit_mask=None, rcond_min=1e-3,
                                   poly_rcond_min=1e-10, chunk_t=None, *, modes=None, grp_start=None, mode_rcond_min=1e-10):
    """The filter-and-bin polarised map of nearest-pixel pointing: for every detector and every scan -- segment
    [seg_start[s], seg_start[s+1]) of the time axis -- a polynomial of degree <= `order` is fitted to the samples that do not look
    at bright sky and subtracted from the whole scan (ops.polyfilter_tod, whose seg_start, order and poly_rcond_min = its
    rcond_min these are), and the filtered timestream is binned: binned_map_pol_nearest_tod of it with the weights `w`, whose
    other arguments, rcond_min and chunk_t these are.  Returns (map, rcond, weights, filtered_tod): what
    binned_map_pol_nearest_tod returns, and the (D, T) filtered timestream.

    fit_mask: an (ny, nx) Float64 plane (Enmap or tensor), None for no mask.  A sample takes part in the fit only where
    fit_mask > 0 at its nearest pixel: the fit weights are w_fit = w * [fit_mask at the sample > 0], built one _TodChunks chunk at
    a time with sample_nearest, so an off-map sample (which samples +0.0) and one whose position is not finite are left out of the
    fit; they are still filtered, and binned or not as binned_map_pol_nearest_tod decides.  With fit_mask=None w_fit = w.  A
    source under a zero of the mask is not fitted away; without the mask the fit takes part of it and the map is biased low around
    it -- the filter is a projection, and this map is not the least-squares map of anything but the filtered data.

    modes (keyword only; None: no such step): the (D, K) or (D,) detector couplings of ops.modefilter_tod, whose
    modes, grp_start and mode_rcond_min = its rcond_min these are.  THE ORDER IS POLYNOMIAL FIRST, THEN MODES: the mode filter
    runs in place on the polynomial-filtered timestream, with the same w_fit, before the binning -- per time sample and detector
    group the modes are fitted to the detectors that are off the masked sky and subtracted from all of them.  The two
    projections do not commute where the cuts differ between detectors, and the result is the second one's: no mode is left in
    any time sample, while a polynomial may be put back at the level of the cuts.  order=None skips the polynomial step
    (seg_start is then not looked at, and may be None): a common-mode-and-bin map.  With modes=None the calls are those made
    without these three arguments.

    Peak extra memory: two (D, T) arrays, w_fit and the filtered timestream (one more while a (D,) `w` is spread over time),
    plus _TodChunks' chunk buffers, which the mask pass and the binning pass share.  tod itself is not changed.  Float64, CAR,
    full maps, one device.  template_bin_map_pol_nearest_tod is this map with the binned templates of DESIGN 4.20 between the two steps."""
    return _filter_bin("filter_bin_map_pol_nearest_tod", tod, w, q_bore, q_det, gamma, shape, wcs, seg_start, order, fit_mask, rcond_min,
                       poly_rcond_min, chunk_t, modes, grp_start, mode_rcond_min, None)


def template_bin_map_pol_nearest_tod(tod, w, q_bore, q_det, gamma, shape, wcs, bins, seg_start=None, order=None, fit_mask=None, rcond_min=1e-3,
                                     poly_rcond_min=1e-10, chunk_t=None, *, modes=None, grp_start=None, mode_rcond_min=1e-10):
    """filter_bin_map_pol_nearest_tod with a binned-template step for scan-synchronous signal -- ground pickup that
    repeats with azimuth, a half-wave plate's synchronous signal, the difference between the sweep directions.  It stands beside
    that function, whose argument list is fixed, and takes its arguments with its meanings; seg_start and order now default to None
    (no polynomial step).  Returns (map, rcond, weights, filtered_tod) as it does.

    bins (None: no such step, and the calls are filter_bin_map_pol_nearest_tod's): the plan of ops.binfilter_tod, either the
    (order, bin_start) pair of ops.bin_plan or an (index, n_bin) pair of a (T,) integer bin index and the number of bins, from
    which the plan is built once.  Per detector and bin -- of azimuth, of scan phase and direction (ops.scan_bins) -- the weighted
    mean of the samples that are off the masked sky is subtracted from all samples of the bin.  THE ORDER IS POLYNOMIAL, THEN
    BINNED TEMPLATE, THEN MODES, each step in place on the previous one's result with the same w_fit.  The projections do not
    commute where their items cut across each other or the cuts differ, and the result is the last one's: its null space is
    exact -- no mode in any time sample with modes, else no mean in any bin -- while an earlier step's signal may be put back at
    the level of the cuts.  order=None with modes=None is allowed when bins is given: a template-and-bin map; with all three
    absent the call is refused."""
    return _filter_bin("template_bin_map_pol_nearest_tod", tod, w, q_bore, q_det, gamma, shape, wcs, seg_start, order, fit_mask, rcond_min,
                       poly_rcond_min, chunk_t, modes, grp_start, mode_rcond_min, bins)


def _filter_bin(what, tod, w, q_bore, q_det, gamma, shape, wcs, seg_start, order, fit_mask, rcond_min, poly_rcond_min, chunk_t, modes, grp_start,
                mode_rcond_min, bins):
    """The two public functions above in the name of `what`: the mask pass, then the polynomial, the binned templates and the modes,
    each where it was asked for, then the binning."""
    ops._car_only(wcs, what)
    rmin = ops._rcond_min(rcond_min)
    if order is None and modes is None and bins is None:
        raise ValueError("%s: order=None skips the polynomial step and needs modes" % what + ("" if what.startswith("filter") else " or bins"))
    source = _TodChunks(what, tod, w, q_bore, q_det, gamma, chunk_t)
    nd, nt = tod.shape
    if bins is not None:
        if not (isinstance(bins, (tuple, list)) and len(bins) == 2):
            raise ValueError("%s: bins is the (order, bin_start) pair of bin_plan or an (index, n_bin) pair" % what)
        if not isinstance(bins[1], torch.Tensor):                       # an index and its number of bins: the plan, built once
            index = ops._bin_index(what, bins[0])
            if index.numel() != nt:
                raise ValueError("%s: the bin index holds one entry per time sample, T = %d" % (what, nt))
            bins = ops.bin_plan(index, bins[1], device=tod.device)
    w_fit = w
    if fit_mask is not None:
        mv = fit_mask.data if isinstance(fit_mask, Enmap) else fit_mask
        ops._no_f32(what, mv, "fit_mask")
        mv = ops._on(ops._dev_f64(mv, "fit_mask"), "fit_mask", tod.device)
        if tuple(mv.shape) != (int(shape[1]), int(shape[0])):
            raise ValueError("%s: fit_mask is one (%d, %d) plane" % (what, shape[1], shape[0]))
        plane = Enmap(mv, wcs)
        w_fit = torch.empty((nd, nt), dtype=torch.float64, device=tod.device)
        for i, (_d, wc, sky, _resp) in enumerate(source.chunks(with_d=False)):
            t0, ct = i * source.chunk_t, wc.numel() // nd
            keep = ops.sample_nearest(plane, sky)[0] > 0
            w_fit[:, t0:t0 + ct] = (wc * keep.to(torch.float64)).reshape(nd, ct)
    if order is not None:
        source.tod = ops.polyfilter_tod(tod, seg_start, order, w=w_fit, rcond_min=poly_rcond_min)
    if bins is not None:
        source.tod = ops.binfilter_tod(source.tod, bins, w=w_fit, out=None if order is None else source.tod)
    if modes is not None:
        source.tod = ops.modefilter_tod(source.tod, modes, w=w_fit, grp_start=grp_start, out=None if order is None and bins is None else source.tod,
                                        rcond_min=mode_rcond_min)
    del w_fit
    return _binned(what, source, shape, wcs, rmin, 0) + (source.tod,)


# ---- the maximum-likelihood map under correlated noise ---------------------------------------------------------------

def ml_map_pol_nearest_tod(tod, w, q_bore, q_det, gamma, shape, wcs, kernel, seg_start=None, rcond_min=1e-3, tol=1e-8, maxiter=200,
                           chunk_t=None):
    """The maximum-likelihood polarised map of nearest-pixel pointing under stationary correlated noise: the m that
    solves (P^T N^-1 P) m = P^T N^-1 d, P the order-0 pointing matrix and N^-1 = G T G the banded-Toeplitz noise weight of
    ops.toeplitz_tod, whose `kernel` ((D, lambda + 1) or (lambda + 1,), on the device of tod; ops.noise_kernel_from_psd makes one)
    and `seg_start` (None: one segment [0, T]) these are.  Where the filters and the destriper project the drift out -- and bias
    the map, or model one offset per baseline -- this weights every sample against its neighbours by the noise's own
    correlation, and is unbiased for any sky.  tod, q_bore, q_det, gamma, chunk_t as for binned_map_pol_nearest_tod; tol and
    maxiter are pcg's.  THE NOISE LEVEL LIVES IN THE KERNEL (c_0 ~ 1 / sigma^2, which must be finite and > 0 for every
    detector): `w`, (D, T) or (D,), ONLY FLAGS -- a sample is live where w > 0 and cut otherwise, whatever the value.

    Returns (map, rcond, weights, info): the (3, ny, nx) IQU Enmap, unsolved pixels +0.0; the (ny, nx) conditioning Enmap; the
    (6, ny, nx) weight planes; pcg's info.  `weights` and `rcond` are those of the WHITE-NOISE diagonal, the pixel blocks of
    P^T diag(c_0 [w > 0]) P: they decide which pixels are solved and are the block-Jacobi preconditioner.  They are NOT the ML
    map's inverse covariance P^T N^-1 P, which couples pixels along every scan and is never formed.

    The passes, over _TodChunks (chunks may cut scans anywhere; the Toeplitz step is never chunked, because its blocks cross
    chunk boundaries): (1) the weight planes of _accumulate at order 0 for the weights c_0[det] [w > 0] (no right-hand side is
    formed: 0 * NaN under a cut would unsolve its pixel) and one pol_block_solve give weights, rcond and mask = (rcond >=
    rcond_min).  (2) g, (D, T): [w > 0] [mask at the sample's nearest pixel > 0], built chunk by chunk with
    sample_nearest as filter_bin_map_pol_nearest_tod builds its fit weights; an off-map sample and one whose position is not
    finite are cut, and so is a sample on an unsolved pixel -- its sky is not modelled, and through T it would leak into its
    neighbours' pixels.  (3) rhs = sum over the chunks of scatter_pol_nearest(u), u = toeplitz_tod(tod, kernel, seg_start, g).
    (4) pcg with A p = sum over the chunks of scatter_pol_nearest(u), u = toeplitz_tod(v, kernel, seg_start, g), v =
    sample_pol_nearest(p) chunk by chunk, and M^-1 = pol_block_solve(., weights, rcond_min).  M^-1 returns +0.0 on an unsolved
    pixel, so p and the map stay exactly +0.0 there in all three planes.  That is iterations + 3 passes over the observation,
    each expanding the pointing again.  With lambda = 0 A is exactly its pixel blocks, M on the solved pixels, and pcg ends
    after one update with binned_map_pol_nearest_tod's map for the weights c_0.

    Peak extra memory: three (D, T) arrays, g, v and u, plus _TodChunks' chunk buffers.  tod is not changed, and its value under
    a cut is never read into a sum.  A NaN or Inf that reaches the right-hand side raises ValueError; "converged" False or
    "breakdown" True in info means the map is not the solution -- a kernel that is not positive semi-definite (a truncation
    without a taper) shows as a breakdown.  Float64, CAR, full maps, one device.  Order 1 is the same driver over sample_pol
    and scatter_pol and is not built."""
    what = "ml_map_pol_nearest_tod"
    ops._car_only(wcs, what)
    rmin = ops._rcond_min(rcond_min)
    source = _TodChunks(what, tod, w, q_bore, q_det, gamma, chunk_t)
    nd, nt = tod.shape
    ops._no_f32(what, kernel, "kernel")
    if not isinstance(kernel, torch.Tensor) or kernel.dim() not in (1, 2) or kernel.shape[-1] < 1 or (kernel.dim() == 2 and kernel.shape[0] != nd):
        raise ValueError("%s: kernel is a (D, lambda + 1) tensor, or (lambda + 1,) for every detector" % what)
    if kernel.shape[-1] - 1 > ops.TOEPLITZ_LAMBDA_MAX:
        raise ValueError("%s: lambda must be 0 to %d, not %d" % (what, ops.TOEPLITZ_LAMBDA_MAX, kernel.shape[-1] - 1))
    seg_start = [0, nt] if seg_start is None else ops._seg_start(what, seg_start, nt)      # checked before the first pass, not in the third
    kernel = ops._on(ops._dev_f64(kernel, "kernel"), "kernel", tod.device)
    c0 = kernel[..., 0].reshape(-1).expand(nd)
    if not bool((torch.isfinite(c0) & (c0 > 0)).all()):
        raise ValueError("%s: kernel[..., 0] = c_0, the inverse noise variance, must be finite and > 0 for every detector" % what)
    flag = (w > 0).to(torch.float64)
    source.w = c0 * flag if w.dim() == 1 else c0[:, None] * flag          # pass 1: the white-noise diagonal
    del flag
    weights = None                                                        # _accumulate's weight planes alone: tod may hold a NaN under a cut,
    for _d, wc, sky, resp in source.chunks(with_d=False):                 # and 0 * NaN in a right-hand side would unsolve its pixel
        weights = ops.scatter_pol_weights_nearest(wc, sky, resp, shape, wcs, out=weights)
    _z, rcond = ops.pol_block_solve(Enmap(torch.zeros_like(weights.data[:3]), wcs), weights, rcond_min=rmin, return_rcond=True)
    mask = Enmap((rcond.data >= rmin).to(torch.float64), wcs)
    del _z

    g = torch.empty((nd, nt), dtype=torch.float64, device=tod.device)     # pass 2: the live samples on solved pixels
    for i, (_d, wc, sky, _resp) in enumerate(source.chunks(with_d=False)):
        t0, ct = i * source.chunk_t, wc.numel() // nd
        keep = (ops.sample_nearest(mask, sky)[0] > 0) & (wc > 0)
        g[:, t0:t0 + ct] = keep.to(torch.float64).reshape(nd, ct)
    u = torch.empty_like(g)

    def scatter_u(y):
        for i, (_d, wc, sky, resp) in enumerate(source.chunks(with_d=False)):
            t0, ct = i * source.chunk_t, wc.numel() // nd
            y = ops.scatter_pol_nearest(u[:, t0:t0 + ct].reshape(-1).contiguous(), sky, resp, shape, wcs, out=y)
        return y

    ops.toeplitz_tod(tod, kernel, seg_start, w=g, out=u)                    # pass 3: P^T N^-1 d
    b = scatter_u(None).data
    if not bool(torch.isfinite(b).all()):
        raise ValueError("%s: P^T N^-1 d is not finite: cut non-finite samples with w = 0" % what)
    v = torch.empty_like(g)

    def apply_a(p):
        pm = Enmap(p, wcs)
        for i, (_d, wc, sky, resp) in enumerate(source.chunks(with_d=False)):
            t0, ct = i * source.chunk_t, wc.numel() // nd
            v[:, t0:t0 + ct] = ops.sample_pol_nearest(pm, sky, resp).reshape(nd, ct)
        ops.toeplitz_tod(v, kernel, seg_start, w=g, out=u)
        return scatter_u(Enmap(torch.zeros_like(p), wcs)).data

    def apply_minv(r):
        return ops.pol_block_solve(Enmap(r, wcs), weights, rcond_min=rmin).data

    x, info = pcg(apply_a, apply_minv, b, tol, maxiter)
    return Enmap(x, wcs), rcond, weights, info


def ml_map_pol_nearest_tod_auto(tod, w, q_bore, q_det, gamma, shape, wcs, lam, seg_start=None, lam_est=None, n_fft=None, n_pass=1,
                                normalise="biased", floor=1e-3, rcond_min=1e-3, tol=1e-8, maxiter=200, chunk_t=None):
    """ml_map_pol_nearest_tod with the noise kernel estimated from the data itself: a self-calibrating ML map.  tod, w
    (which only flags), q_bore, q_det, gamma, shape, wcs, seg_start, rcond_min, tol, maxiter and chunk_t are
    ml_map_pol_nearest_tod's; lam, lam_est, n_fft, normalise and floor are ops.noise_kernel_from_tod's.  Returns (map, rcond,
    weights, info, noise): the first three as ml_map_pol_nearest_tod returns them for the last pass; info the last pass's pcg
    info plus "passes", the list of every pass's info, pass 0 included; noise a dict of the last pass's "kernel" ((D, lam + 1), on
    the device), "psd", "n_floored" (host arrays), "sums" and "pairs" (on the device).

    The steps: (1) pass 0, ml_map_pol_nearest_tod with the kernel [1.0]: at lambda = 0 that is the binned map of the flags [w > 0]
    after one CG update, and it never reads a NaN under a cut.  (2) Chunk by chunk over _TodChunks, with sample_nearest and
    sample_pol_nearest as filter_bin_map_pol_nearest_tod builds its fit weights: g = [w > 0] [rcond >= rcond_min at the
    sample's pixel], and the residual tod - P m, (D, T), +0.0 where g is 0 so that a NaN under a cut stays where it is.  (3)
    kernel = the composition of ops.noise_kernel_from_tod on (residual, lam, seg_start, w=g, lam_est, n_fft, normalise, floor).
    (4) ml_map_pol_nearest_tod with that kernel.  Steps 2 to 4 run n_pass >= 1 times, each from the previous pass's map.

    WHAT THIS IS NOT.  The residual of a binned map is not the noise: the map has absorbed the part of the noise that projects
    onto the pixels, so the residual UNDERESTIMATES the noise, most on thinly hit pixels (a pixel hit once has residual 0), and
    the estimate is of one realisation, smoothed over 2 pi / (lam_est + 1) by the taper.  It is not an unbiased spectrum and no
    substitute for a noise model where there is one; it is the weight that makes the ML map available without one.  Measured on
    the ML test case (1/f noise, five seeds, lam = lam_est = 64, n_fft = 4096, the dense numpy solve), rms map error:

        seed    binned map    ML, TRUE kernel    ML, ESTIMATED kernel    (second pass)
        11      0.590         0.426              0.389                   0.377
        12      0.702         0.548              0.546                   0.549
        13      0.432         0.307              0.328                   0.330
        14      0.643         0.558              0.540                   0.534
        15      0.552         0.367              0.365                   0.372

    below the binned map in five of five, within 7 % of the true kernel's, cond(A) 6.1 to 6.3, nothing floored; a second pass
    changes nothing worth having, hence n_pass = 1.  Peak extra memory: ml_map_pol_nearest_tod's three (D, T) arrays, and two
    more, g and the residual, between its calls.  Float64, CAR, full maps, one device."""
    what = "ml_map_pol_nearest_tod_auto"
    if isinstance(n_pass, bool) or not isinstance(n_pass, int) or n_pass < 1:
        raise ValueError("%s: n_pass must be an integer >= 1, not %r" % (what, n_pass))
    lam = ops._lam(what, lam)
    lam_est = lam if lam_est is None else ops._lam(what, lam_est)
    if normalise not in ("biased", "pairs"):
        raise ValueError("%s: normalise is \"biased\" or \"pairs\", not %r" % (what, normalise))
    if n_fft is not None and (int(n_fft) <= 2 * lam_est or int(n_fft) // 2 < lam):
        raise ValueError("%s: n_fft must exceed 2 lam_est = %d and reach 2 lam = %d, not %r" % (what, 2 * lam_est, 2 * lam, n_fft))
    ops._car_only(wcs, what)
    rmin = ops._rcond_min(rcond_min)
    source = _TodChunks(what, tod, w, q_bore, q_det, gamma, chunk_t)         # every argument check of the passes, before the first
    nd, nt = tod.shape
    segs = [0, nt] if seg_start is None else ops._seg_start(what, seg_start, nt)
    common = dict(seg_start=segs, rcond_min=rcond_min, tol=tol, maxiter=maxiter, chunk_t=chunk_t)
    white = torch.ones((1,), dtype=torch.float64, device=tod.device)
    m, rcond, weights, info = ml_map_pol_nearest_tod(tod, w, q_bore, q_det, gamma, shape, wcs, white, **common)
    passes, noise = [info], {}
    mask = Enmap((rcond.data >= rmin).to(torch.float64), wcs)
    for _ in range(n_pass):
        g = torch.empty((nd, nt), dtype=torch.float64, device=tod.device)
        res = torch.empty_like(g)
        for i, (d, wc, sky, resp) in enumerate(source.chunks()):
            t0, ct = i * source.chunk_t, wc.numel() // nd
            keep = (ops.sample_nearest(mask, sky)[0] > 0) & (wc > 0)
            g[:, t0:t0 + ct] = keep.to(torch.float64).reshape(nd, ct)
            r = d - ops.sample_pol_nearest(m, sky, resp)
            res[:, t0:t0 + ct] = torch.where(keep, r, torch.zeros_like(r)).reshape(nd, ct)
        sums, pairs = ops.autocov_tod(res, lam_est, segs, g)
        del res, g
        psd, n_floored = ops.noise_psd_from_autocov(sums, pairs, n_fft, normalise, floor)
        kernel = ops.noise_kernel_from_psd(psd, lam).to(tod.device)
        noise = {"kernel": kernel, "psd": psd, "sums": sums, "pairs": pairs, "n_floored": n_floored}
        m, rcond, weights, info = ml_map_pol_nearest_tod(tod, w, q_bore, q_det, gamma, shape, wcs, kernel, **common)
        passes.append(info)
    info = dict(info)
    info["passes"] = passes
    return m, rcond, weights, info, noise


# ---- the destriper ----------------------------------------------------------------------------------------------------

def destripe_map_pol_nearest_tod(tod, w, q_bore, q_det, gamma, shape, wcs, baseline_len, rcond_min=1e-3, tol=1e-8, maxiter=200,
                                 chunk_t=None):
    """The destriped polarised map of nearest-pixel pointing: the model d = P m + F a + n, P the order-0 pointing
    matrix, n white noise of weights w, F one offset per detector and `baseline_len` consecutive samples (n_base =
    ceil(T / baseline_len) baselines per detector, the last one possibly short).  With M = P^T W P (exactly the pixel blocks at
    order 0) and Z = I - P M^-1 P^T W the offsets solve

        (F^T W Z F) a = F^T W Z d,      and the map is      m = M^-1 P^T W (d - F a),

    M^-1 being pol_block_solve with its rule (unsolved pixels +0.0).  tod, w, q_bore, q_det, gamma, chunk_t as for
    binned_map_pol_nearest_tod; tol and maxiter are pcg's.  Returns (map, rcond, weights, baselines, info): the (3, ny, nx) IQU
    Enmap, the (ny, nx) conditioning Enmap and the (6, ny, nx) weight planes of binned_map_pol_nearest_tod, the (D, n_base)
    offsets, and pcg's info.

    The passes, each over _TodChunks (a chunk's t0 is its index times chunk_t; chunks may cut baselines anywhere):
    _accumulate at order 0 and one pol_block_solve give the binned map m_d and rcond; mask = (rcond >= rcond_min), and a sample
    on a masked pixel is cut from every later pass, so it neither pulls its baseline toward a zero sky nor enters the map;
    b = sum of baseline_project_pol_nearest(d, m=m_d); the preconditioner s = sum of baseline_project_pol_nearest(a=1), the
    weight each baseline carries, M^-1 r = r / s where s > 0 and +0.0 elsewhere; A p = baseline_bin_pol_nearest(a=p) into a
    zeroed map, pol_block_solve against the saved weights, baseline_project_pol_nearest(a=p, m=that); pcg; and the map is
    pol_block_solve(sum of baseline_bin_pol_nearest(d, a), weights).  That is 2 * iterations + 4 passes over the observation,
    each expanding the pointing again, and nothing of size D * T is held besides tod and w.

    THE GAUGE.  A constant added to every baseline of a set of baselines connected through shared pixels cannot be told from a
    constant added to I on those pixels: F^T W Z F is positive SEMI-definite with one zero eigenvalue per connected set, and I
    is fixed only up to one constant per set.  CG started from zero never leaves the operator's range, so `baselines` are the
    solution without a component along those null vectors, and the map's I offset is whatever goes with it: compare I after
    removing its mean over the solved pixels.  Q and U are not affected.  A right-hand side that is exactly zero (pcg's
    rz0 == 0) returns zero baselines, and the map is then the binned map of the uncut samples.  A timestream WITHOUT offsets
    leaves a right-hand side of rounding alone, whose null-space part is as large as the rest of it: the baselines then come
    back as one constant that is not small (0.65 in the test case) plus rounding -- pure gauge, it moves only the mean of I.

    A baseline all of whose samples are cut has s = 0 and stays +0.0.  A NaN or Inf that reaches rhs raises ValueError
    (_accumulate): cut non-finite samples with w = 0 and a finite d; a NaN or all-zero quaternion cuts its samples by itself.
    "converged" False or "breakdown" True in info means the baselines are not the solution.  Float64, CAR, full maps, one device."""
    what = "destripe_map_pol_nearest_tod"
    ops._car_only(wcs, what)
    rmin = ops._rcond_min(rcond_min)
    blen = int(baseline_len)
    if blen < 1:
        raise ValueError("%s: baseline_len must be at least 1" % what)
    source = _TodChunks(what, tod, w, q_bore, q_det, gamma, chunk_t)
    nd, nt = tod.shape
    nb = -(-nt // blen)
    rhs, weights = _accumulate(what, source, shape, wcs, 0)
    m_d, rcond = ops.pol_block_solve(rhs, weights, rcond_min=rmin, out=rhs, return_rcond=True)
    mask = (rcond.data >= rmin).to(torch.float64)

    def project(with_d, a, m):
        out = torch.zeros((nd * nb,), dtype=torch.float64, device=tod.device)
        for i, (d, wc, sky, resp) in enumerate(source.chunks(with_d=with_d)):
            ops.baseline_project_pol_nearest(wc, sky, resp, shape, wcs, nd, i * source.chunk_t, blen, nb, d=d, a=a, m=m, mask=mask, out=out)
        return out

    def bin_solve(with_d, a):
        y = None
        for i, (d, wc, sky, resp) in enumerate(source.chunks(with_d=with_d)):
            y = ops.baseline_bin_pol_nearest(wc, sky, resp, shape, wcs, nd, i * source.chunk_t, blen, nb, d=d, a=a, mask=mask, out=y)
        return ops.pol_block_solve(y, weights, rcond_min=rmin, out=y)

    b = project(True, None, m_d)
    s = project(False, torch.ones_like(b), None)
    live = s > 0

    def apply_a(p):
        return project(False, p, bin_solve(False, p))

    def apply_minv(r):
        return torch.where(live, r / s, torch.zeros_like(r))

    a, info = pcg(apply_a, apply_minv, b, tol, maxiter)
    return bin_solve(True, a), rcond, weights, a.reshape(nd, nb), info
