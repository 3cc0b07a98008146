"""Shared pieces of the GP.extend tests: the bordered Cholesky factorisation in numpy (the algebra gpx_gp_extend runs on the
device, checked against numpy's own factorisation in tests/test_extend_cpu.py), the test cases with their oracle -- one
CPU evaluation per (kind, n + k), never modified -- and small device buffers for the two gpx_d_* kernels."""
import ctypes

import numpy as np

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from oracle import gp_oracle as orc
from _ard_helpers import iso_params

ARD_W = (0.7, 1.1, 1.6)
M_TEST = 50


def bordered_cholesky(K, n):
    """Lower Cholesky factor of the symmetric positive definite K from the factor of its leading n x n block:
    L' = [[L, 0], [X, Ls]] with X = B L^-T and Ls Ls^T = C - X X^T, where K = [[A, B^T], [B, C]]."""
    K = np.asarray(K, dtype=np.float64)
    N = K.shape[0]
    L = np.linalg.cholesky(K[:n, :n])
    X = np.linalg.solve(L, K[n:, :n].T).T
    out = np.zeros((N, N))
    out[:n, :n] = L
    out[n:, :n] = X
    out[n:, n:] = np.linalg.cholesky(K[n:, n:] - X @ X.T)
    return out


def make_kernel(kind):
    if kind == "gaussian":
        return gp.GaussianKernel(1.0, 0.5 * np.sqrt(3))
    if kind == "periodic":
        return gp.PeriodicKernel(1.0, 0.8, 3.0)
    return gp.GaussianARDKernel(1.0, list(ARD_W))


_CASES = {}


def case(kind, total):
    """(x, y, xo, oracle) for `total` points of `kind` in {"gaussian" (d = 3), "periodic" (d = 1), "ard" (d = 3, unequal
    widths)}, s = 1.  The oracle of the ARD family is the Gaussian one on x / w with (h / sqrt(wbar), 1), as in
    tests/_ard_helpers.py; `oracle.xo` are the test points in the oracle's own coordinates."""
    if (kind, total) not in _CASES:
        d = 1 if kind == "periodic" else 3
        X, y, Xo = orc.synth_inputs(total, d, M_TEST)
        if kind == "periodic":
            perm = np.random.RandomState(7).permutation(total)      # synth_inputs sorts 1-D inputs: the new points are not the largest
            X, y = X[perm], y[perm]
            o = orc.OracleGP("periodic", (1.0, 0.8, 3.0), X, y, 1.0)
            o.xo = Xo
        elif kind == "gaussian":
            o = orc.OracleGP("gaussian", (1.0, 0.5 * np.sqrt(3)), X, y, 1.0)
            o.xo = Xo
        else:
            w = np.asarray(ARD_W)
            o = orc.OracleGP("gaussian", iso_params(1.0, w), X / w, y, 1.0)
            o.xo = Xo / w
        if d == 1:
            X, Xo = X.ravel(), Xo.ravel()
        _CASES[(kind, total)] = (X, y, Xo, o)
    return _CASES[(kind, total)]


def close(got, ref, rel=1e-10):
    """|got - ref| <= rel * max|ref|: two fp64 device evaluations of one quantity (the bound of tests/test_gpu_dist_cov.py)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err, bound = float(np.abs(got - ref).max()), rel * float(np.abs(ref).max())
    print("device vs device: err %.3e bound %.3e" % (err, bound))
    assert got.shape == ref.shape
    assert err <= bound, "|got - ref| = %.3e exceeds %.0e max|ref| = %.3e" % (err, rel, bound)


class DeviceBuffers(object):
    """gpx_malloc'ed blocks, freed on exit."""

    def __init__(self):
        self.lib = _lib.load()
        self.bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.gpx_device_sync()
        for b in self.bufs:
            self.lib.gpx_free(b)

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        b = ctypes.c_void_p()
        _lib.check(self.lib.gpx_malloc(ctypes.byref(b), max(arr.nbytes, 16)))
        self.bufs.append(b)
        _lib.check(self.lib.gpx_memcpy_h2d(b, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes, None))
        return b

    def get(self, b, like):
        _lib.check(self.lib.gpx_device_sync())
        out = np.empty_like(like)
        _lib.check(self.lib.gpx_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), b, out.nbytes, None))
        return out
