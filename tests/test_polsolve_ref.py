"""tests/polsolve_ref.py, the yardstick of the per-pixel IQU block solve, held to independent definitions:
LAPACK's solve, numpy's eigenvalues, the rank of a sum of fewer than three p p^T, and A @ x.  CPU only."""
import numpy as np
import pytest

import polsolve_ref as Q

N = 120000
LEVELS = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8)


@pytest.fixture(scope="module")
def blocks():
    w6, r3, hits = Q.random_blocks(N, 0)
    return w6, r3, hits


def _rel_inf(x, ref):
    """max |x - ref| / max |ref| per block, (3, n) inputs."""
    return np.abs(x - ref).max(axis=0) / np.abs(ref).max(axis=0)


def test_against_lapack_and_the_eigenvalues(blocks):
    """Every block accepted at rcond_min = 1e-8 agrees with np.linalg.solve within polsolve_ref.C_LAPACK * 2^-52 / rc in relative
    infinity norm (C_LAPACK = 532 is derived above its definition: the backward errors of LDL^T and of LAPACK's LU, carried
    forward with kappa_inf <= 3 / rc), and its rc is at least lambda_min / lambda_max of np.linalg.eigvalsh, less 1e-12
    relative.  The largest rc / (lambda_min / lambda_max) is printed; DESIGN 4.13 records it."""
    w6, r3, hits = blocks
    x, rc, info = Q.solve(w6, r3, 1e-8)
    ok = info["ok"]
    assert ok.sum() > N // 2
    assert np.array_equal(rc > 0, rc != 0) and np.all(rc[ok] >= 1e-8) and np.all(rc <= 1.0)
    A = Q.dense(w6[:, ok])
    ref = np.linalg.solve(A, r3[:, ok].T[:, :, None])[:, :, 0].T
    err = _rel_inf(x[:, ok], ref) * rc[ok] / Q.EPS
    print("solve against LAPACK on %d accepted blocks: worst error * rc / 2^-52 = %.3g (bound %g)" % (int(ok.sum()), float(err.max()), Q.C_LAPACK))
    assert np.all(err <= Q.C_LAPACK)
    lam = np.linalg.eigvalsh(A)
    ratio = lam[:, 0] / lam[:, 2]
    assert np.all(rc[ok] >= ratio * (1 - 1e-12))
    print("rc / (lambda_min / lambda_max): %.6g to %.6g" % (float((rc[ok] / ratio).min()), float((rc[ok] / ratio).max())))


def test_rank_deficient_blocks_are_never_accepted(blocks):
    """A sum of fewer than three w p p^T has rank below 3: not accepted at any rcond_min from 1e-2 to 1e-8, zeros in all three
    planes.  So that this is not vacuous, at least 40 % of all blocks have three or more hits and are accepted at 1e-6."""
    w6, r3, hits = blocks
    few = hits < 3
    assert few.sum() > N // 5
    for level in LEVELS:
        x, rc, info = Q.solve(w6, r3, level)
        assert not info["ok"][few].any(), "a block of fewer than three hits accepted at rcond_min = %g" % level
        assert not x[:, few].any() and not np.signbit(x[:, few]).any()
        assert np.all(rc[few] < 1e-12) and not np.signbit(rc[few]).any()
        if level == 1e-6:
            share = float((info["ok"] & (hits >= 3)).mean())
            print("accepted at 1e-6 with >= 3 hits: %.1f %% of the blocks; largest rc below three hits: %.3g" % (100 * share, float(rc[few].max())))
            assert share >= 0.40
    # zero hits is the zero block
    none = hits == 0
    assert none.any() and not w6[:, none].any()


def _is_plus_zero(a):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.zeros(np.shape(a), np.int64))


@pytest.mark.parametrize("level", [1e-3, 1e-6, 1.0])
def test_special_blocks_give_zeros_and_rcond_zero(level):
    """The zero block, NaN / +Inf / -Inf in any one of the nine inputs, a zero or negative largest diagonal entry and -0.0
    entries: three +0.0 and rcond +0.0, as bit patterns."""
    names, w6, r3 = Q.special_blocks()
    assert len(names) == 2 + 27 + 7
    x, rc, info = Q.solve(w6, r3, level)
    for k, name in enumerate(names):
        assert not info["ok"][k], name
        assert _is_plus_zero(x[:, k]), "%s: %r" % (name, x[:, k])
        assert _is_plus_zero(rc[k]), "%s: rcond %r" % (name, rc[k])
    # the block the non-finite cases spoil is solved when left alone
    xg, rcg, ig = Q.solve(np.array(Q.GOOD)[:, None], np.array(Q.GOOD_RHS)[:, None], 1e-3)
    assert ig["ok"][0] and rcg[0] > 0.3
    assert np.allclose(Q.dense(np.array(Q.GOOD)[:, None])[0] @ xg[:, 0], Q.GOOD_RHS, rtol=1e-14)


def test_ties_on_the_diagonal_pick_the_first():
    names, w6, r3, i1 = Q.tie_blocks()
    x, rc, info = Q.solve(w6, r3, 1e-3)
    assert np.array_equal(info["i1"], i1) and info["ok"].all()
    ref = np.linalg.solve(Q.dense(w6), r3.T[:, :, None])[:, :, 0].T
    assert np.all(_rel_inf(x, ref) <= Q.C_LAPACK * Q.EPS / rc)
    assert np.array_equal(x[:, 0], np.array(Q.GOOD_RHS)) and rc[0] == 1.0       # the identity
    # a tie in the second pivot keeps the order too: s22 = s33 does not swap
    assert not info["swap"][0]


def test_permutation_invariance(blocks):
    """Relabelling I, Q, U relabels the solution: both are within 45 * 2^-52 / rc of the exact solution (the LDL^T half of
    C_LAPACK's derivation), so within C_LAPACK * 2^-52 / rc of each other; rc may move, both are held to the smaller one."""
    w6, r3, hits = blocks
    w6, r3 = w6[:, :30000], r3[:, :30000]
    x, rc, info = Q.solve(w6, r3, 1e-6)
    for perm in Q.PERMS:
        p = list(perm)
        wp, rp = Q.relabel(w6, r3, perm)
        xp, rcp, ip = Q.solve(wp, rp, 1e-6)
        both = info["ok"] & ip["ok"]
        assert both.sum() > 12000
        err = _rel_inf(xp[:, both], x[p][:, both]) * np.minimum(rc, rcp)[both] / Q.EPS
        print("permutation %s: worst gap * rc / 2^-52 = %.3g" % (perm, float(err.max())))
        assert np.all(err <= Q.C_LAPACK)
        # a block accepted under one labelling only sits at the threshold
        edge = info["ok"] != ip["ok"]
        assert np.all(np.maximum(rc, rcp)[edge] < 1e-5)


def test_apply_and_the_round_trip(blocks):
    """apply() against A @ x: two summation orders of three products, each within gamma_3 |A||x|, so 3 * 2^-52 |A||x| apart.
    solve(apply(x)) returns x on accepted blocks: apply's rounding is one more backward error of at most gamma_3 |A| <= 9u ||A||_inf
    beside the 30u ||A||_inf of the solve, well inside C_LAPACK."""
    w6, r3, hits = blocks
    w6, x0 = w6[:, :30000], r3[:, :30000]
    A = Q.dense(w6)
    y = Q.apply(w6, x0)
    want = (A @ x0.T[:, :, None])[:, :, 0].T
    scale = (np.abs(A) @ np.abs(x0).T[:, :, None])[:, :, 0].T
    assert np.all(np.abs(y - want) <= 3 * Q.EPS * scale)
    back, rc, info = Q.solve(w6, y, 1e-6)
    ok = info["ok"]
    assert ok.sum() > 12000
    err = _rel_inf(back[:, ok], x0[:, ok]) * rc[ok] / Q.EPS
    print("solve(apply(x)) on %d blocks: worst error * rc / 2^-52 = %.3g" % (int(ok.sum()), float(err.max())))
    assert np.all(err <= Q.C_LAPACK)
    assert not back[:, ~ok].any()


def test_mixed_blocks_hold_every_special_block_and_every_pivot_order():
    """What the device tests feed the kernel: every special block, and SOLVED blocks in each of the six (first pivot, second-pivot
    swap) classes, so that every select of the permutation and of the un-permutation is compared with a non-zero value."""
    names, sw, sr = Q.special_blocks()
    for npix in (255, 257, 512, 65160):
        w6, r3 = Q.mixed_blocks(npix)
        assert w6.shape == (6, npix) and r3.shape == (3, npix)
        assert np.array_equal(w6[:, 2:2 + len(names)].view(np.int64), sw.view(np.int64))
        for level in (1e-3, 1e-6):
            x, rc, info = Q.solve(w6, r3, level)
            for i1 in (0, 1, 2):
                for swap in (False, True):
                    n = int((info["ok"] & (info["i1"] == i1) & (info["swap"] == swap) & (x != 0).all(axis=0)).sum())
                    assert n >= 5, "npix %d, rcond_min %g: %d solved blocks with first pivot %d, swap %s" % (npix, level, n, i1, swap)
    w6, r3 = Q.mixed_blocks(2)
    assert Q.solve(w6, r3, 1e-3)[2]["ok"].any()
