"""The least-squares polarised map-maker: preconditioned conjugate gradients on the normal equations
P^T W P m = P^T W d, with the per-pixel IQU blocks that scatter_pol_weights accumulates as the preconditioner.

pcg() is the iteration alone, on torch tensors of any device: it calls nothing of the library, only the two operators it is
given.  cg_map_pol() builds those operators from ops.normal_pol (or the composition scatter_pol(w * sample_pol(.))),
ops.scatter_pol_weights and ops.pol_block_solve.

binned_map_pol_nearest() is the map-maker of nearest-pixel (order 0) pointing, where P^T W P is exactly its pixel
blocks: one pass over the samples and one pol_block_solve, no iteration."""
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
