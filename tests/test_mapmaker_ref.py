"""pj.pcg on torch CPU tensors against tests/normal_ref.py: A = P^T W P as a scipy.sparse matrix, M^-1 the block
solve of polsolve_ref, the least-squares map from a sparse direct solve.  No GPU and no library call: pcg is the iteration alone.

The bars.  With lambda_min <= lambda <= lambda_max the eigenvalues of the pencil (A, M), kappa = lambda_max / lambda_min, r the
recursive residual at the stop and e = x - x* the error, r = -A e in exact arithmetic and
    |e|_A^2 = r^T A^-1 r <= r^T M^-1 r / lambda_min,       |x*|_A^2 = b^T A^-1 b >= b^T M^-1 b / lambda_max,
so the stopping rule r^T M^-1 r <= tol^2 b^T M^-1 b gives |e|_A <= sqrt(kappa) tol |x*|_A.  Rounding moves the recursive residual
off the true one by ~kappa * 2^-53 relative, four orders below the bar at tol = 1e-8.  The iteration cap is
normal_ref.iteration_cap: the Chebyshev bound carried into the stopping norm, plus five."""
import numpy as np
import pytest

import normal_ref as NR

torch = pytest.importorskip("torch")

GEOMS = ["box_2x2", "box_5x7", "box_24x12", "cc_90x46"]


def _run(pj, c, b, tol, maxiter=200):
    A = c.A
    x, info = pj.pcg(lambda p: torch.from_numpy(A @ p.numpy()), lambda r: torch.from_numpy(c.minv(r.numpy())),
                     torch.from_numpy(np.ascontiguousarray(b)), tol, maxiter)
    return x.numpy(), info


@pytest.mark.parametrize("tol", [1e-4, 1e-8])
@pytest.mark.parametrize("geom", GEOMS)
def test_pcg_meets_the_a_norm_bound_and_the_iteration_cap(pj, O, geom, tol):
    c = NR.case(pj, O, geom)
    assert c.solved.all(), "at least 48 points per pixel: every pixel block is accepted"
    assert len(c.w) >= 48 * c.shape[0] * c.shape[1]
    xs = c.direct(c.d)
    x, info = _run(pj, c, c.rhs(c.d), tol)
    kappa, cap = c.kappa, NR.iteration_cap(c.kappa, tol)
    err, bar = c.anorm(x - xs), np.sqrt(kappa) * tol * c.anorm(xs)
    print("%s tol %g: kappa = %.3g, %d iterations (cap %d), |x - x*|_A / bound = %.3g" % (geom, tol, kappa, info["iterations"], cap, err / bar))
    assert info["converged"] and not info["breakdown"]
    assert len(info["history"]) == info["iterations"] and info["history"][-1] <= tol
    assert err <= bar
    assert info["iterations"] <= cap


@pytest.mark.parametrize("geom", GEOMS + ["box_80x40"])
def test_noiseless_samples_recover_the_sky_and_the_binned_map_does_not(pj, O, geom):
    c = NR.case(pj, O, geom)
    m0 = c.m0.ravel()
    top = np.abs(m0).max()
    x, info = _run(pj, c, c.rhs(c.d0), 1e-10)
    cg, binned = np.abs(x - m0).max(), np.abs(c.binned(c.d0) - m0).max()
    print("%s: max|x - m0| = %.3g after %d iterations, binned map off by %.3g, max|m0| = %.3g" % (geom, cg, info["iterations"], binned, top))
    assert info["converged"]
    assert cg <= 1e-6 * top
    assert binned > 0.1 * top


def test_masked_pixels_stay_zero_and_the_rest_converges(pj, O):
    """The (90, 46) map with points only in pixel rows [10, 36]: the yardstick of tests/test_gpu_mapmaker.py's masked case, held
    to the same cap.  Rows 1-8 and 38-46 take no hit: unsolved, and exactly +0.0 in x."""
    c = NR.case(pj, O, "cc_90x46", masked=True)
    nx, ny = c.shape
    solved = c.solved.reshape(ny, nx)
    assert not solved[:8].any() and not solved[37:].any() and solved[10:35].all()
    tol = 1e-8
    x, info = _run(pj, c, c.rhs(c.d), tol)
    cap = NR.iteration_cap(c.kappa, tol)
    xs = c.direct(c.d)
    err, bar = c.anorm(x - xs), np.sqrt(c.kappa) * tol * c.anorm(xs)
    print("masked: kappa = %.3g, %d iterations (cap %d), |x - x*|_A / bound = %.3g, %d of %d pixels solved" % (
        c.kappa, info["iterations"], cap, err / bar, int(solved.sum()), solved.size))
    assert info["converged"] and info["iterations"] <= cap and err <= bar
    dead = ~np.tile(c.solved, 3)
    assert np.array_equal(x[dead].view(np.int64), np.zeros(int(dead.sum()), np.int64)), "an unsolved pixel is not +0.0"


def test_zero_right_hand_side(pj):
    x, info = pj.pcg(lambda p: 2 * p, lambda r: r.clone(), torch.zeros((3, 4, 5), dtype=torch.float64), 1e-8, 10)
    assert x.shape == (3, 4, 5) and not x.any()
    assert info == {"iterations": 0, "converged": True, "breakdown": False, "history": []}


def test_negative_definite_operator_breaks_down(pj):
    b = torch.arange(1.0, 7.0, dtype=torch.float64)
    x, info = pj.pcg(lambda p: -p, lambda r: r.clone(), b, 1e-8, 10)
    assert info["breakdown"] and not info["converged"] and info["iterations"] == 0 and info["history"] == []
    assert not x.any()


def test_maxiter_is_honoured(pj, O):
    c = NR.case(pj, O, "box_24x12")
    x, info = _run(pj, c, c.rhs(c.d), 1e-8, maxiter=3)
    assert not info["converged"] and not info["breakdown"] and info["iterations"] == 3 and len(info["history"]) == 3
    assert all(np.isfinite(info["history"])) and info["history"][-1] > 1e-8 and np.isfinite(x).all()


def test_nan_in_b_raises(pj):
    b = torch.ones(12, dtype=torch.float64)
    b[5] = float("nan")
    with pytest.raises(ValueError):
        pj.pcg(lambda p: 2 * p, lambda r: r.clone(), b, 1e-8, 10)
    with pytest.raises(ValueError):                                   # an M^-1 that is not positive definite
        pj.pcg(lambda p: 2 * p, lambda r: -r, torch.ones(12, dtype=torch.float64), 1e-8, 10)
    with pytest.raises(TypeError):
        pj.pcg(lambda p: 2 * p, lambda r: r.clone(), torch.ones(12, dtype=torch.float32), 1e-8, 10)
