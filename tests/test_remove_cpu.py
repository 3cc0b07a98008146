"""CPU tests of GP.remove: the numpy restatement of the factor deletion the GPU tests lean on, the binding of the two new
symbols and the two new counters, and the refusals that come before the library is touched."""
import os
import re
from ctypes import POINTER, c_int, c_int64, c_void_p

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from _extend_helpers import case
from _remove_helpers import SHAPES, SHAPE_IDS, cholesky_delete

c_int_p = POINTER(c_int)
_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "gpx.h")


@pytest.mark.parametrize("n,idx", [(n, idx) for n, idx, _ in SHAPES if n <= 520] + [(300, [299, 0, 150]), (700, list(range(40)))],
                         ids=[i for i, (n, _, _) in zip(SHAPE_IDS, SHAPES) if n <= 520] + ["n300_unsorted", "n700_k40_oldest"])
def test_cholesky_delete_equals_numpy(n, idx):
    """1e-12 max|ref| against the 1.5e-15 the rotations measure at these condition numbers (cond(K) <= 570)."""
    K = case("gaussian", n)[3].Kxx
    L = np.linalg.cholesky(K)
    keep = np.setdiff1d(np.arange(n), idx)
    ref = np.linalg.cholesky(K[np.ix_(keep, keep)])
    got = cholesky_delete(L, idx)
    err, bound = float(np.abs(got - ref).max()), 1e-12 * float(np.abs(ref).max())
    print("cholesky_delete vs numpy: err %.3e bound %.3e" % (err, bound))
    assert got.shape == ref.shape and err <= bound
    assert np.array_equal(np.triu(got, 1), np.zeros_like(got))
    r0 = min(idx)
    assert np.array_equal(got[:, :r0], L[keep][:, :r0])          # the columns before the first deleted one are not touched


def test_cholesky_delete_joint_equals_sequential():
    L = np.linalg.cholesky(case("gaussian", 300)[3].Kxx)
    joint = cholesky_delete(L, [7, 120])
    seq = cholesky_delete(cholesky_delete(L, [7]), [119])
    assert np.abs(joint - seq).max() <= 1e-12 * np.abs(seq).max()


def test_remove_symbols_are_bound():
    want = {
        "gpx_d_chol_delete": (c_int, [c_int, c_void_p, c_int64, c_int64, POINTER(c_int64), c_int64, c_void_p, c_int64, c_void_p]),
        "gpx_gp_remove": (c_int, [c_void_p, POINTER(c_int64), c_int64, POINTER(c_void_p), c_int_p]),
    }
    text = open(_HEADER).read()
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name][0] is res
        assert list(_lib._SIGNATURES[name][1]) == args, name
        assert re.search(r"^int %s\(" % name, text, re.M), name
    assert (_lib.ROUTE_REMOVE, _lib.PROF_CHOL_DELETE) == (24, 18)
    for macro, value in (("GPX_ROUTE_REMOVE", 24), ("GPX_PROF_CHOL_DELETE", 18)):
        assert re.search(r"^#define %s\s+%d\b" % (macro, value), text, re.M), macro


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


@pytest.mark.parametrize("idx", [
    [], np.zeros(0, dtype=np.int64), np.zeros(10, dtype=bool),     # nothing to remove
    [3, 3], [3, -7], [0, 10 - 10, 4],                              # twice, also after normalisation
    10, -11, [0, 10], [-11],                                       # out of range
    list(range(10)), np.ones(10, dtype=bool),                      # all n points
    2.0, [1.0, 2.0], np.array([1.5]), ["a"], None,                 # not integers
    np.ones(9, dtype=bool), np.ones((10, 1), dtype=bool),          # a mask of the wrong shape
    np.zeros((2, 2), dtype=np.int64),                              # not 1-D
], ids=["empty_list", "empty_array", "empty_mask", "twice", "twice_negative", "twice_zero", "n", "below_minus_n", "n_in_list",
        "below_minus_n_in_list", "all_points", "all_points_mask", "float", "float_list", "float_array", "string", "none",
        "short_mask", "mask_2d", "ints_2d"])
def test_remove_refuses_before_the_library(no_library, idx):
    rng = np.random.RandomState(0)
    g = gp.GP(gp.GaussianKernel(1.0, 1.0), rng.randn(10, 3), rng.randn(10), s=1.0)
    with pytest.raises(ValueError):
        g.remove(idx)


def test_remove_normalises_indices(no_library):
    g = gp.GP(gp.GaussianKernel(1.0, 1.0), np.linspace(0, 1, 10), np.zeros(10), s=1.0)
    for idx, want in [(3, [3]), (-1, [9]), ([5, -10, 2], [0, 2, 5]), (range(3), [0, 1, 2]), (np.int32(4), [4]),
                      (np.arange(10) % 4 == 1, [1, 5, 9]), (np.array([7, 1], dtype=np.uint8), [1, 7])]:
        got = g._removal_indices(idx)
        assert got.dtype == np.int64 and got.flags.c_contiguous and got.tolist() == want


def test_distributed_gp_refuses_remove(no_library):
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    dist = gp.DistributedGP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1)
    assert gp.DistributedGP.remove is not gp.GP.remove          # refused, not the single-GPU path inherited
    with pytest.raises(NotImplementedError):
        dist.remove(0)
