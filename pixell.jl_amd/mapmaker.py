"""The least-squares polarised map-maker: preconditioned conjugate gradients on the normal equations
P^T W P m = P^T W d, with the per-pixel IQU blocks that scatter_pol_weights accumulates as the preconditioner.

pcg() is the iteration alone, on torch tensors of any device: it calls nothing of the library, only the two operators it is
given.  cg_map_pol() builds those operators from ops.normal_pol (or the composition scatter_pol(w * sample_pol(.))),
ops.scatter_pol_weights and ops.pol_block_solve.

binned_map_pol_nearest() is the map-maker of nearest-pixel (order 0) pointing, where P^T W P is exactly its pixel
blocks: one pass over the samples and one pol_block_solve, no iteration.

binned_map_pol_nearest_tod() and cg_map_pol_tod() are the same two map-makers from a (D, T) time-ordered data array and the
telescope's pointing as quaternions: ops.expand_pointing produces the coordinates and responses one time chunk
at a time into two reused buffers, so the 32 B per sample of expanded pointing never exist for the whole observation."""
import math

import torch

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


def cg_map_pol(batches, shape, wcs, rcond_min=1e-3, tol=1e-8, maxiter=200, fused=True):
    """The least-squares polarised map: the m that minimises |W^(1/2) (d - P m)|, P the order-1 pointing matrix of sample_pol and
    W diagonal, by block-Jacobi-preconditioned CG on P^T W P m = P^T W d.  `batches` is a sequence of
    (d, w, skycoords, resp): (N,) samples and weights, (N, 2) coordinates and responses, as for binned_map_pol.  Returns
    (map, rcond, info): the (3, ny, nx) IQU Enmap, the (ny, nx) conditioning Enmap of the pixel blocks, and pcg's info.

    rhs = P^T W d and the six weight planes are accumulated over the batches with out=, as in binned_map_pol's recipe; rcond
    comes from one pol_block_solve; M^-1 = pol_block_solve(., weights, rcond_min); A p starts from a zeroed map and takes
    normal_pol(p, w, skycoords, resp, out=...) for every batch.  fused=False forms A p as scatter_pol(w * sample_pol(p))
    instead: the same terms bit for bit, three launches and an N-length temporary per batch.  On the MI355X (10^8 points on
    a 43200 x 21601 x 3 map) the fused call was 1.30-1.35x faster than that composition on sphere-uniform points and level with
    it (1.02x) on raster-ordered ones.

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

    A NaN or Inf that reaches rhs raises ValueError: non-finite samples are the caller's to cut, with w = 0 AND a finite d
    (0 * NaN is NaN).  Order 1 only, for binned_map_pol's reason; Float64, CAR, one device."""
    from . import ops
    batches = list(batches)
    if not batches:
        raise ValueError("cg_map_pol needs at least one batch (d, w, skycoords, resp)")
    rmin = ops._rcond_min(rcond_min)
    for bt in batches:
        if len(bt) != 4:
            raise ValueError("a batch is (d, w, skycoords, resp)")
        ops._sample_vectors("cg_map_pol", bt[0], bt[1])
    rhs = weights = None
    for d, w, sky, resp in batches:
        rhs = ops.scatter_pol(w * d, sky, resp, shape, wcs, order=1, out=rhs)
        weights = ops.scatter_pol_weights(w, sky, resp, shape, wcs, order=1, out=weights)
    if not bool(torch.isfinite(rhs.data).all()):
        raise ValueError("cg_map_pol: P^T W d is not finite: cut non-finite samples with w = 0 and a finite d")
    _z, rcond = ops.pol_block_solve(rhs, weights, rcond_min=rmin, return_rcond=True)

    def apply_a(p):
        y = torch.zeros_like(p)
        pm = Enmap(p, wcs)
        for _d, w, sky, resp in batches:
            if fused:
                ops.normal_pol(pm, w, sky, resp, out=y)
            else:
                ops.scatter_pol(w * ops.sample_pol(pm, sky, resp), sky, resp, shape, wcs, out=y)
        return y

    def apply_minv(r):
        return ops.pol_block_solve(Enmap(r, wcs), weights, rcond_min=rmin).data

    x, info = pcg(apply_a, apply_minv, rhs.data, tol, maxiter)
    return Enmap(x, wcs), rcond, info


def binned_map_pol_nearest(batches, shape, wcs, rcond_min=1e-3, fused=True):
    """The polarised map of nearest-pixel (order 0) pointing: one pass over the samples and one per-pixel solve, no
    iteration.  `batches` is a sequence of (d, w, skycoords, resp) as for cg_map_pol.  Returns (map, rcond, weights): the
    (3, ny, nx) IQU Enmap, the (ny, nx) conditioning Enmap of the pixel blocks, and the (6, ny, nx) Enmap of the weight planes
    II, IQ, IU, QQ, QU, UU.

    Every batch takes one bin_pol_nearest into rhs = P^T W d and the six weight planes, then one
    pol_block_solve(..., return_rcond=True) turns them into the map.  fused=False accumulates with
    scatter_pol_nearest(w * d) and scatter_pol_weights_nearest(w) instead: the same terms bit for bit, two launches, a torch
    multiply and an N-length temporary per batch.  On the MI355X (10^8 points on a 43200 x 21601 x 3 map) the fused call took
    43.7 ms on sphere-uniform points and 24.6 ms on raster-ordered ones against 44.2 and 25.2 ms for that composition: level, the
    nine atomics per point being all of either form's time.

    With nearest-pixel pointing every sample touches one pixel, so P^T W P has no entries outside the per-pixel 3 x 3 blocks:
    `weights` is EXACTLY P^T W P, which for white noise of variance 1 / w is the inverse covariance of the map, and this map
    IS the least-squares map for this P -- the m that minimises |W^(1/2) (d - P m)| on the solved pixels -- where the order-1
    binned_map_pol only inverts the diagonal blocks of a coupled system.  That is why order 0 has no CG map-maker and no
    normal-operator kernel: pol_block_apply(x, weights) is P^T W P x.

    Unsolved pixels (pol_block_solve's rule: no hits, fewer than three, one polarisation angle, a pivot ratio below
    rcond_min) are +0.0 in the map; cut on the returned rcond.  A NaN or Inf that reaches rhs raises ValueError, as in
    cg_map_pol: non-finite samples are the caller's to cut, with w = 0 AND a finite d.  Float64, CAR, full maps, one device."""
    from . import ops
    batches = list(batches)
    if not batches:
        raise ValueError("binned_map_pol_nearest needs at least one batch (d, w, skycoords, resp)")
    ops._car_only(wcs, "binned_map_pol_nearest")
    rmin = ops._rcond_min(rcond_min)
    for bt in batches:
        if len(bt) != 4:
            raise ValueError("a batch is (d, w, skycoords, resp)")
        for t, noun in zip(bt, ("d", "w", "skycoords", "resp")):
            ops._no_f32("binned_map_pol_nearest", t, noun)
        ops._sample_vectors("binned_map_pol_nearest", bt[0], bt[1])
    rhs = weights = None
    for d, w, sky, resp in batches:
        if fused:
            rhs, weights = ops.bin_pol_nearest(d, w, sky, resp, shape, wcs, rhs=rhs, weights=weights)
        else:
            rhs = ops.scatter_pol_nearest(w * d, sky, resp, shape, wcs, out=rhs)
            weights = ops.scatter_pol_weights_nearest(w, sky, resp, shape, wcs, out=weights)
    if not bool(torch.isfinite(rhs.data).all()):
        raise ValueError("binned_map_pol_nearest: P^T W d is not finite: cut non-finite samples with w = 0 and a finite d")
    m, rcond = ops.pol_block_solve(rhs, weights, rcond_min=rmin, out=rhs, return_rcond=True)
    return m, rcond, weights


# ---- the same map-makers from time-ordered data and quaternion pointing, expanded chunk by chunk ----------------

def _tod_args(what, tod, w, q_bore, q_det, gamma, chunk_t):
    """The checks the two _tod map-makers share; returns chunk_t.  tod is (D, T); w is (D, T) or (D,); q_bore (T, 4), q_det (D, 4)
    and gamma ((D,) or None) are expand_pointing's, which checks them itself on the first chunk."""
    from . import ops
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
    return min(chunk_t, nt)


def _tod_chunks(tod, w, q_bore, q_det, gamma, chunk_t, with_d=True):
    """Yields (d, w, skycoords, resp) of the time chunks [t0, t0 + chunk_t) of a (D, T) observation, detector-major as
    expand_pointing writes them.  skycoords and resp are views of two buffers of chunk_t * D pairs that every chunk reuses: a
    chunk is to be consumed (on the current stream) before the next is asked for.  d and w are the chunk's samples and weights
    made contiguous (copies, unless the chunk is the whole observation); d is None without with_d."""
    from . import ops
    nd, nt = tod.shape
    sky_buf = torch.empty((nd * chunk_t, 2), dtype=torch.float64, device=tod.device)
    resp_buf = torch.empty_like(sky_buf)
    for t0 in range(0, nt, chunk_t):
        ct = min(chunk_t, nt - t0)
        sky, resp = ops.expand_pointing(q_bore[t0:t0 + ct], q_det, gamma, out_sky=sky_buf[:nd * ct], out_resp=resp_buf[:nd * ct])
        d = tod[:, t0:t0 + ct].reshape(-1).contiguous() if with_d else None      # (a one-sample chunk reshapes to a strided view)
        wc = (w[:, t0:t0 + ct] if w.dim() == 2 else w[:, None].expand(nd, ct)).reshape(-1).contiguous()
        yield d, wc, sky, resp


def binned_map_pol_nearest_tod(tod, w, q_bore, q_det, gamma, shape, wcs, rcond_min=1e-3, chunk_t=None):
    """binned_map_pol_nearest from time-ordered data and quaternion pointing.  tod: the (D, T) samples of D
    detectors; w: their weights, (D, T) or one per detector (D,); q_bore (T, 4), q_det (D, 4), gamma ((D,) or None): the
    arguments of expand_pointing.  The observation is taken in time chunks of chunk_t samples per detector (None: 2^24 // D):
    each chunk is expanded into two reused buffers and passed to bin_pol_nearest(rhs=, weights=); one pol_block_solve ends the
    job.  Returns (map, rcond, weights) as binned_map_pol_nearest does, and raises what it raises.  Peak extra memory is
    32 * D * chunk_t bytes of expanded pointing, plus 16 * D * chunk_t for the contiguous copies of the chunk's samples and
    weights.  A boresight or detector quaternion that is NaN, Inf or all zeros cuts its samples (their position is NaN and
    bin_pol_nearest adds nothing for them).  The accumulation order of the atomics differs from the batch form's, so the two
    maps agree to the scatters' rounding clause, not to the bit."""
    from . import ops
    what = "binned_map_pol_nearest_tod"
    ops._car_only(wcs, what)
    rmin = ops._rcond_min(rcond_min)
    chunk_t = _tod_args(what, tod, w, q_bore, q_det, gamma, chunk_t)
    rhs = weights = None
    for d, wc, sky, resp in _tod_chunks(tod, w, q_bore, q_det, gamma, chunk_t):
        rhs, weights = ops.bin_pol_nearest(d, wc, sky, resp, shape, wcs, rhs=rhs, weights=weights)
    if not bool(torch.isfinite(rhs.data).all()):
        raise ValueError("%s: P^T W d is not finite: cut non-finite samples with w = 0 and a finite d" % what)
    m, rcond = ops.pol_block_solve(rhs, weights, rcond_min=rmin, out=rhs, return_rcond=True)
    return m, rcond, weights


def cg_map_pol_tod(tod, w, q_bore, q_det, gamma, shape, wcs, rcond_min=1e-3, tol=1e-8, maxiter=200, chunk_t=None):
    """cg_map_pol (order 1) from time-ordered data and quaternion pointing; arguments as for
    binned_map_pol_nearest_tod, tol and maxiter as for cg_map_pol.  rhs = P^T W d and the six weight planes are accumulated
    chunk by chunk; every application of the normal operator expands each chunk again and takes normal_pol on it, so the
    expansion kernel runs (iterations + 2) times over the observation and nothing of size D * T is ever held besides tod and
    w.  pcg is the iteration, unchanged.  Returns (map, rcond, info) as cg_map_pol does, and raises what it raises."""
    from . import ops
    what = "cg_map_pol_tod"
    ops._car_only(wcs, what)
    rmin = ops._rcond_min(rcond_min)
    chunk_t = _tod_args(what, tod, w, q_bore, q_det, gamma, chunk_t)
    rhs = weights = None
    for d, wc, sky, resp in _tod_chunks(tod, w, q_bore, q_det, gamma, chunk_t):
        rhs = ops.scatter_pol(wc * d, sky, resp, shape, wcs, order=1, out=rhs)
        weights = ops.scatter_pol_weights(wc, sky, resp, shape, wcs, order=1, out=weights)
    if not bool(torch.isfinite(rhs.data).all()):
        raise ValueError("%s: P^T W d is not finite: cut non-finite samples with w = 0 and a finite d" % what)
    _z, rcond = ops.pol_block_solve(rhs, weights, rcond_min=rmin, return_rcond=True)

    def apply_a(p):
        y = torch.zeros_like(p)
        pm = Enmap(p, wcs)
        for _d, wc, sky, resp in _tod_chunks(tod, w, q_bore, q_det, gamma, chunk_t, with_d=False):
            ops.normal_pol(pm, wc, sky, resp, out=y)
        return y

    def apply_minv(r):
        return ops.pol_block_solve(Enmap(r, wcs), weights, rcond_min=rmin).data

    x, info = pcg(apply_a, apply_minv, rhs.data, tol, maxiter)
    return Enmap(x, wcs), rcond, info
