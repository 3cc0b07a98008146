"""Shared pieces of the GP.remove tests: the deletion of rows and columns from a Cholesky factor in numpy (the algebra
gpx_d_chol_delete runs on the device, checked against numpy's own factorisation in tests/test_remove_cpu.py), the (n, idx)
shapes of the GPU tests, and the oracle on the kept rows -- one CPU evaluation per (kind, n, idx), never modified."""
import numpy as np

from oracle import gp_oracle as orc
from _ard_helpers import iso_params
from _extend_helpers import ARD_W, case


def cholesky_delete(L, idx):
    """Lower Cholesky factor of K with the rows and columns `idx` deleted, from the lower factor L of K = L L^T.

    `idx`: distinct indices, sorted here.  The columns before min(idx) are kept as they are; behind a deleted column the
    factor takes the rank-1 update L33' L33'^T = L33 L33^T + l32 l32^T by Givens rotations.  All updates share one pass: the
    columns ascend, and in one column the update vectors born so far are applied in ascending order; a deleted column,
    rotated by the vectors born before it, becomes the next vector.  Equal to deleting the points one after another."""
    L = np.array(L, dtype=np.float64)
    n = L.shape[0]
    rm = np.sort(np.asarray(idx, dtype=np.int64).ravel())
    k = rm.size
    assert k >= 1 and rm[0] >= 0 and rm[-1] < n and np.all(rm[1:] > rm[:-1])
    V = np.zeros((n, k))
    born = 0
    for j in range(int(rm[0]), n):
        for r in range(born):
            a, b = L[j, j], V[j, r]
            rho = np.sqrt(a * a + b * b)
            c, s = a / rho, b / rho
            lcol, vcol = L[j:, j].copy(), V[j:, r].copy()
            L[j:, j] = c * lcol + s * vcol
            V[j:, r] = c * vcol - s * lcol
        if born < k and rm[born] == j:
            V[j + 1:, born] = L[j + 1:, j]
            born += 1
    keep = np.setdiff1d(np.arange(n), rm)
    return np.tril(L[np.ix_(keep, keep)])


def _random_indices(n, k, seed):
    return sorted(int(i) for i in np.random.RandomState(seed).choice(n, k, replace=False))


# the smallest shapes at which the deletion kernel can still go wrong: (n, idx, what it covers)
SHAPES = [
    (2, [0], "smallest n, the whole factor updated"),
    (2, [1], "the last point only: nothing to rotate, pure truncation"),
    (65, [0], "three column blocks, a ragged last one"),
    (65, [64], "the last point only"),
    (520, [0, 31, 32, 63, 64, 127, 128, 255, 256, 257, 519], "every block edge for widths 32 .. 256, births inside and at the ends of blocks, the last row"),
    (300, list(range(0, 300, 2)), "k = 150: more vectors than any group"),
    (1990, _random_indices(1990, 37, 11), "ragged last block, several row bands"),
]
SHAPE_IDS = ["n%d_k%d_from%d" % (n, len(idx), idx[0]) for n, idx, _ in SHAPES]
HANDLE_SHAPES = [(n, idx) for n, idx, _ in SHAPES if n >= 300]
HANDLE_IDS = [i for i, (n, _, _) in zip(SHAPE_IDS, SHAPES) if n >= 300]

_KEPT = {}


def kept_case(kind, n, idx):
    """(x, y, xo, oracle) of case(kind, n) and the oracle fitted on the rows that `idx` keeps."""
    x, y, xo, full = case(kind, n)
    key = (kind, n, tuple(idx))
    if key not in _KEPT:
        xk, yk = np.delete(x, idx, axis=0), np.delete(y, idx)
        if kind == "periodic":
            o = orc.OracleGP("periodic", (1.0, 0.8, 3.0), xk.reshape(-1, 1), yk, 1.0)
        elif kind == "gaussian":
            o = orc.OracleGP("gaussian", (1.0, 0.5 * np.sqrt(3)), xk, yk, 1.0)
        else:
            w = np.asarray(ARD_W)
            o = orc.OracleGP("gaussian", iso_params(1.0, w), xk / w, yk, 1.0)
        o.xo = full.xo
        _KEPT[key] = o
    return x, y, xo, _KEPT[key]
