"""CPU tests of GP.extend: the binding of the four new symbols, the numpy restatement of the bordered factorisation the GPU
tests lean on, and the shape refusals that come before the library is touched."""
from ctypes import POINTER, c_double, c_int, c_int64, c_void_p

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from _extend_helpers import bordered_cholesky

c_double_p, c_int_p = POINTER(c_double), POINTER(c_int)


def test_extend_symbols_are_bound():
    want = {
        "gpx_gp_extend": (c_int, [c_void_p, c_double_p, c_double_p, c_int64, POINTER(c_void_p), c_int_p]),
        "gpx_gp_extend_from_K": (c_int, [c_void_p, c_double_p, c_double_p, c_int64, c_double_p, c_double_p, POINTER(c_void_p),
                                         c_int_p]),
        "gpx_d_copy_lower": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p]),
        "gpx_d_schur_lower": (c_int, [c_int, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    }
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name][0] is res
        assert list(_lib._SIGNATURES[name][1]) == args, name
    assert _lib.ROUTE_EXTEND == 19


def test_bordered_cholesky_equals_numpy():
    rng = np.random.RandomState(3)
    n, k = 60, 5
    x = rng.uniform(-3, 3, (n + k, 2))
    K = np.exp(-0.5 * ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)) + np.eye(n + k)
    L = bordered_cholesky(K, n)
    ref = np.linalg.cholesky(K)
    assert np.abs(L - ref).max() <= 1e-12
    assert np.array_equal(L[:n, :n], np.linalg.cholesky(K[:n, :n]))     # the old rows are the old factor
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L))


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


@pytest.mark.parametrize("x_new,y_new", [
    (np.zeros((2, 4)), np.zeros(2)),            # wrong d
    (np.zeros(2), np.zeros(2)),                 # (k,) for 3-D inputs
    (np.zeros((2, 3)), np.zeros(3)),            # y_new of the wrong length
    (np.zeros((2, 3)), np.zeros((2, 1))),       # y_new not (k,)
    (np.zeros((0, 3)), np.zeros(0)),            # k = 0
    (np.zeros((2, 3, 1)), np.zeros(2)),         # x_new 3-D
], ids=["wrong_d", "x_1d", "y_length", "y_2d", "k0", "x_3d"])
def test_extend_refuses_bad_shapes_before_the_library(no_library, x_new, y_new):
    rng = np.random.RandomState(0)
    g = gp.GP(gp.GaussianKernel(1.0, 1.0), rng.randn(10, 3), rng.randn(10), s=1.0)
    with pytest.raises(ValueError):
        g.extend(x_new, y_new)


def test_extend_refuses_bad_shapes_1d(no_library):
    g = gp.GP(gp.GaussianKernel(1.0, 1.0), np.linspace(0, 1, 10), np.zeros(10), s=1.0)
    for x_new, y_new in [(np.zeros((2, 1)), np.zeros(2)), (np.zeros(0), np.zeros(0)), (np.zeros(2), np.zeros(1))]:
        with pytest.raises(ValueError):
            g.extend(x_new, y_new)


def test_distributed_gp_refuses_extend(no_library):
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    dist = gp.DistributedGP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1)
    assert gp.DistributedGP.extend is not gp.GP.extend          # refused, not the single-GPU path inherited
    with pytest.raises(NotImplementedError):
        dist.extend(np.zeros(1), np.zeros(1))
