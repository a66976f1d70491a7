"""What the yardsticks of the two timestream filters (polyfilter_ref.py, modefilter_ref.py) share, as csrc/pxl_fit.h holds it for the
device: the clamped items, the xor tree that joins the lanes' sums, and the dense projector.  The two `solve`s are NOT here: they are
two independent transcriptions of one definition, and tests/test_modefilter_ref.py holds them to the same bits."""
import numpy as np


def clamp(starts, n):
    """[(lo, hi)] of every fitted item after both ends are clamped to [0, n]; hi == lo for an empty one."""
    s = [min(max(int(v), 0), n) for v in starts]
    return [(s[k], max(s[k + 1], s[k])) for k in range(len(s) - 1)]


def tree(v):
    """v_l = v_l + v_(l ^ off) along the first axis for off = len / 2, ..., 1: lane 0's value (every lane ends with the same bits)."""
    off = len(v) // 2
    while off > 0:
        v = v + v[np.arange(len(v)) ^ off]
        off //= 2
    return v[0]


def projector(F, w):
    """The dense (n, n) matrix Z = I - F (F^T W F)^-1 F^T W of one full-rank item of n samples, F its (n, K) basis in long double."""
    F = np.asarray(F, dtype=np.longdouble).reshape(len(w), -1)
    W = np.diag(np.asarray(w, dtype=np.longdouble))
    A = (F.T @ W @ F).astype(np.float64)
    return np.eye(len(w)) - (F.astype(np.float64) @ np.linalg.solve(A, (F.T @ W).astype(np.float64)))
