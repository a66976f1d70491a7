"""numpy yardstick for the per-pixel IQU block solve and block product (pxl_pol_block_solve_f64 / pxl_pol_block_apply_f64,
pj.pol_block_solve / pj.pol_block_apply), CPU only.

solve() is the contract of include/pixell_hip.h written with array operations in exactly its order: LDL^T with diagonal
pivoting, every product, quotient, sum and difference a separate numpy operation (one rounding each, nothing fuses), every
choice an np.where on the comparisons the contract names.  The device must give these BITS.  tests/test_polsolve_ref.py holds
this file to LAPACK and to numpy's eigenvalues.

a, b, c, d, e, f are the weight planes II, IQ, IU, QQ, QU, UU: A = [a b c; b d e; c e f]."""
import numpy as np

EPS = 2.0 ** -52

# Relative error of solve() against np.linalg.solve, in units of 2^-52 / rc (u = 2^-53, n = 3; Higham, Accuracy and Stability
# of Numerical Algorithms, 2nd ed., Theorems 9.4 and 10.4):
#   ours     (A + dA) x = b with |dA| <= gamma_{3n+1} |L||D||L^T|.  On a positive semi-definite block every entry of |L||D||L^T| is
#            at most sqrt(a_ii a_jj) <= p1 <= ||A||_inf (Cauchy-Schwarz on the rows of |L| D^(1/2)), so ||dA||_inf <= 3 * 10u ||A||_inf.
#   LAPACK   LU with partial pivoting: |dA| <= gamma_{3n} |L||U|, |l_ij| <= 1 and |u_ij| <= rho max|a_ij| with the growth factor
#            rho <= 2^(n-1) = 4, so || |L||U| ||_inf <= n^2 rho ||A||_inf and ||dA||_inf <= 9u * 36 ||A||_inf = 324u ||A||_inf.
#   forward  ||x^ - x||_inf / ||x||_inf <= kappa_inf ||dA||_inf / ||A||_inf to first order, kappa_inf <= 3 kappa_2 (symmetric A:
#            sqrt(3) each for ||A|| and ||A^-1||) and kappa_2 = lambda_max / lambda_min <= 1 / rc (p3 >= lambda_min, p1 <= lambda_max).
#   total    3 (30 + 324) u / rc = 1062 u / rc = 531 * 2^-52 / rc; one more covers the second-order terms (rc >= 1e-8 here).
C_LAPACK = 532.0


def solve(w6, r3, rcond_min):
    """w6 (6, n), r3 (3, n).  Returns (x (3, n), rcond (n,), info): info holds ok, i1 and swap per block."""
    a, b, c, d, e, f = (np.asarray(w6[k], dtype=np.float64) for k in range(6))
    r0, r1, r2 = (np.asarray(r3[k], dtype=np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        # first pivot
        f0 = (a >= d) & (a >= f)
        f1 = ~f0 & (d >= f)
        i1 = np.where(f0, 0, np.where(f1, 1, 2))
        m11 = np.where(f0, a, np.where(f1, d, f))
        m21 = np.where(f0, b, np.where(f1, b, c))
        m31 = np.where(f0, c, e)
        m22 = np.where(f0, d, a)
        m32 = np.where(f0, e, np.where(f1, c, b))
        m33 = np.where(f0, f, np.where(f1, f, d))
        R1 = np.where(f0, r0, np.where(f1, r1, r2))
        R2 = np.where(f0, r1, r0)
        R3 = np.where(f0, r2, np.where(f1, r2, r1))
        # first elimination
        p1 = m11
        l21 = m21 / p1
        l31 = m31 / p1
        s22 = m22 - l21 * m21
        s33 = m33 - l31 * m31
        s32 = m32 - l31 * m21
        # second pivot
        swap = s33 > s22
        s22, s33 = np.where(swap, s33, s22), np.where(swap, s22, s33)
        l21, l31 = np.where(swap, l31, l21), np.where(swap, l21, l31)
        R2, R3 = np.where(swap, R3, R2), np.where(swap, R2, R3)
        # second elimination
        p2 = s22
        l32 = s32 / p2
        p3 = s33 - l32 * s32
        # conditioning
        rc2 = p2 / p1
        rc3 = p3 / p1
        rc = np.where(rc3 < rc2, rc3, rc2)
        fin = np.isfinite(r0) & np.isfinite(r1) & np.isfinite(r2)
        ok = fin & (p1 > 0) & (rc2 >= rcond_min) & (rc3 >= rcond_min)
        pos = fin & (p1 > 0) & (rc2 > 0) & (rc3 > 0)
        # solve
        y1 = R1
        y2 = R2 - l21 * y1
        y3 = (R3 - l31 * y1) - l32 * y2
        x3 = y3 / p3
        x2 = y2 / p2 - l32 * x3
        x1 = (y1 / p1 - l21 * x2) - l31 * x3
        # un-permute
        xa = np.where(swap, x3, x2)
        xb = np.where(swap, x2, x3)
        x = np.stack([np.where(ok, np.where(f0, x1, xa), 0.0),
                      np.where(ok, np.where(f0, xa, np.where(f1, x1, xb)), 0.0),
                      np.where(ok, np.where(f0 | f1, xb, x1), 0.0)])
        rcond = np.where(pos, rc, 0.0)
    return x, rcond, {"ok": ok, "i1": i1, "swap": swap}


def apply(w6, x3):
    """The block product, (3, n): each row (m0 * x0 + m1 * x1) + m2 * x2, left to right."""
    a, b, c, d, e, f = (np.asarray(w6[k], dtype=np.float64) for k in range(6))
    x0, x1, x2 = (np.asarray(x3[k], dtype=np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        return np.stack([(a * x0 + b * x1) + c * x2, (b * x0 + d * x1) + e * x2, (c * x0 + e * x1) + f * x2])


def dense(w6):
    """(n, 3, 3) symmetric matrices of the (6, n) planes."""
    a, b, c, d, e, f = w6
    return np.stack([np.stack([a, b, c], -1), np.stack([b, d, e], -1), np.stack([c, e, f], -1)], -2)


def random_blocks(n, seed=0):
    """n blocks as a pointing matrix makes them: sums of 0-11 terms w p p^T, p = (1, cos 2 psi, sin 2 psi), formed as
    pol_ref.terms forms them (t1 = q w, t2 = u w, q t1, q t2, u t2), weights 10^U(-3, 3).  A third of the blocks draw their
    angles in a cluster psi0 +- 10^U(-5, -0.5) rad, the others uniformly; blocks of at least three hits draw all weights within
    one decade half of the time.  Returns (w6 (6, n), r3 (3, n), hits (n,)): a standard normal right-hand side."""
    rng = np.random.default_rng(seed)
    hits = rng.integers(0, 12, n)
    clustered = rng.random(n) < 1.0 / 3
    psi = rng.uniform(0, np.pi, (11, n))
    tight = rng.uniform(0, np.pi, n) + 10.0 ** rng.uniform(-5, -0.5, n) * rng.uniform(-1, 1, (11, n))
    psi = np.where(clustered, tight, psi)
    lw = rng.uniform(-3, 3, (11, n))
    narrow = rng.random(n) < 0.5
    lw = np.where(narrow, lw[0] + lw / 6, lw)
    w = np.where(np.arange(11)[:, None] < hits, 10.0 ** lw, 0.0)
    q, u = np.cos(2 * psi), np.sin(2 * psi)
    t1, t2 = q * w, u * w
    w6 = np.stack([t.sum(axis=0) for t in (w, t1, t2, q * t1, q * t2, u * t2)])
    return w6, rng.normal(size=(3, n)), hits


GOOD = (4.0, 0.5, -0.25, 2.0, 0.125, 3.0)            # a well-conditioned block: strictly diagonally dominant
GOOD_RHS = (1.0, -2.0, 0.5)


def special_blocks():
    """Blocks that must come out as three zeros with rcond +0.0, as (names, w6 (6, n), r3 (3, n)): the zero block; NaN, +Inf
    and -Inf in each of the nine inputs of an otherwise well-conditioned block; a largest diagonal entry that is zero or
    negative; blocks of -0.0."""
    names, w, r = [], [], []

    def add(name, w6, r3=GOOD_RHS):
        names.append(name); w.append(w6); r.append(r3)
    add("zero block", (0.0,) * 6)
    add("zero block, zero rhs", (0.0,) * 6, (0.0,) * 3)
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(9):
            v = list(GOOD + GOOD_RHS)
            v[k] = bad
            add("%r in input %d" % (bad, k), tuple(v[:6]), tuple(v[6:]))
    add("largest diagonal entry zero", (0.0, 0.5, 0.25, -1.0, 0.125, -2.0))
    add("all diagonal entries negative", (-4.0, 0.5, -0.25, -2.0, 0.125, -3.0))
    add("largest diagonal entry negative, equal", (-1.0, 0.0, 0.0, -1.0, 0.0, -1.0))
    add("every entry -0.0", (-0.0,) * 6, (-0.0,) * 3)
    add("diagonal -0.0", (-0.0, 0.0, 0.0, -0.0, 0.0, -0.0))
    add("one -0.0 on the diagonal of a rank-2 block", (1.0, 0.0, 0.0, 1.0, 0.0, -0.0))
    add("-0.0 off the diagonal of the zero block", (0.0, -0.0, -0.0, 0.0, -0.0, 0.0))
    return names, np.array(w, dtype=np.float64).T.copy(), np.array(r, dtype=np.float64).T.copy()


def tie_blocks():
    """Ties on the diagonal, which pick the first of equals, as (names, w6, r3, i1): the identity, a = d > f, d = f > a."""
    names = ["identity", "a = d > f", "d = f > a"]
    w = [(1.0, 0.0, 0.0, 1.0, 0.0, 1.0), (3.0, 0.5, 0.25, 3.0, -0.5, 2.0), (1.0, 0.25, -0.5, 2.0, 0.5, 2.0)]
    return names, np.array(w).T.copy(), np.tile(np.array(GOOD_RHS)[:, None], (1, 3)), np.array([0, 0, 1])


PERMS = ((1, 0, 2), (2, 0, 1), (0, 2, 1), (1, 2, 0), (2, 1, 0))      # the five relabellings of (I, Q, U) other than the identity


def relabel(w6, r3, perm):
    """The same systems with I, Q, U relabelled: A' = A[perm][:, perm], r' = r[perm]; the solution is x[perm]."""
    p = list(perm)
    A = dense(np.asarray(w6))[:, p][:, :, p]
    return np.stack([A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]]), np.asarray(r3)[p]


N_RELABEL_HEAD, N_RELABEL_TAIL = 30, 1000


def mixed_blocks(npix, n_random=65536, seed=0):
    """The device tests' inputs, (w6 (6, npix), r3 (3, npix)): two random blocks, every special block, the ties, 30 random blocks
    that rcond_min = 1e-3 accepts under each of the five relabellings PERMS, then random blocks, 1000 of them under each
    relabelling, cut or cycled to npix.  random_blocks always has II on top (II = sum w >= QQ, UU), so only the relabelled
    blocks put the first pivot on index 1 or 2: with them all six (first pivot, second-pivot swap) classes hold solved blocks
    within the first 255 (tests/test_polsolve_ref.py asserts it)."""
    w, r, _hits = random_blocks(n_random, seed)
    _n, sw, sr = special_blocks()
    _n, tw, tr, _i = tie_blocks()
    good = np.flatnonzero(solve(w, r, 1e-3)[2]["ok"])[:len(PERMS) * N_RELABEL_HEAD]
    head = [relabel(w[:, good[k::len(PERMS)]], r[:, good[k::len(PERMS)]], perm) for k, perm in enumerate(PERMS)]
    w, r = w.copy(), r.copy()
    for k, perm in enumerate(PERMS):
        sl = slice(2000 + k * N_RELABEL_TAIL, 2000 + (k + 1) * N_RELABEL_TAIL)
        w[:, sl], r[:, sl] = relabel(w[:, sl], r[:, sl], perm)
    w6 = np.concatenate([w[:, :2], sw, tw] + [h[0] for h in head] + [w[:, 2:]], axis=1)
    r3 = np.concatenate([r[:, :2], sr, tr] + [h[1] for h in head] + [r[:, 2:]], axis=1)
    at = np.arange(npix) % w6.shape[1]
    return np.ascontiguousarray(w6[:, at]), np.ascontiguousarray(r3[:, at])
