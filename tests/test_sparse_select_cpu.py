"""CPU tests of the greedy selection of inducing points: the ABI's declarations, the Python refusals that fire without a device,
and the numpy restatement of tests/_sparse_select_helpers.py that tests/test_gpu_sparse_select.py holds the device to --
pinned here against what a pivoted partial Cholesky must satisfy and against the restated bound of tests/_sparse_helpers.py."""
import os
import re
from ctypes import POINTER, c_double, c_int, c_int64

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from conftest import ROOT
from oracle import gp_oracle as orc
from _sparse_helpers import oracle_view
from _sparse_select_helpers import (CASES, CASE_IDS, DUP, E32R, FP64_PICKS, FULL, ONE, SEEDS, TABLE, WELL, auto_tol, case_data, elbo_at,
                                    free, greedy, k0_of, kind_of, make_kernel)


def test_abi_is_declared_and_mirrored():
    want = (c_int, [c_int, c_int, POINTER(c_double), c_int64, c_int, POINTER(c_double), c_int64, c_double, c_int64,
                    POINTER(c_int64), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int64)])
    assert "gpx_sgp_select" in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGNATURES["gpx_sgp_select"][0] is want[0]
    assert list(_lib._SIGNATURES["gpx_sgp_select"][1]) == want[1]
    with open(os.path.join(ROOT, "include", "gpx.h")) as f:
        hdr = f.read()
    assert re.search(r"int gpx_sgp_select\(int dtype, int kernel, const double \*x, int64_t n, int d, const double \*params,\s*"
                     r"int64_t m_max, double tol, int64_t first,\s*"
                     r"int64_t \*index, double \*pivot, double \*trace, double \*R, int64_t \*count\);", hdr)
    assert _lib.PROF_SELECT == 22 and re.search(r"#define GPX_PROF_SELECT\s+22\b", hdr)
    assert _lib.ROUTE_SELECT_STEP == 26 and re.search(r"#define GPX_ROUTE_SELECT_STEP\s+26\b", hdr)
    assert (_lib.PROF_SPARSE_ZGRAD, _lib.ROUTE_SPARSE_CHUNK) == (21, 25)          # the ids that were there keep their numbers
    with open(os.path.join(ROOT, "gaussian_processes_amd", "csrc", "Makefile")) as f:
        srcs = re.search(r"^SRCS = (.*)$", f.read(), re.M).group(1).split()
    assert "gpx_select.hip" in srcs
    assert _lib.load().gpx_sgp_select.argtypes == want[1]                         # (resolves it in the built library)
    assert hasattr(gp.SparseGP, "greedy_inducing") and not hasattr(gp, "greedy_inducing")


def test_python_refusals_before_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    x = case_data(FULL)[0]
    K = gp.GaussianKernel(1.0, 2.0)
    greedy_inducing = gp.SparseGP.greedy_inducing

    class Plugin(gp.Kernel):
        pass
    with pytest.raises(NotImplementedError, match="plugin kernels are not supported"):
        greedy_inducing(Plugin(), x, 4)
    for M in (0, -1, 41):
        with pytest.raises(ValueError, match="invalid value for M"):
            greedy_inducing(K, x, M)
    for tol in (-1e-3, np.inf, np.nan):
        with pytest.raises(ValueError, match="invalid value for tol"):
            greedy_inducing(K, x, 4, tol=tol)
    for first in (-1, 40, 2.5):
        with pytest.raises(ValueError, match="invalid value for first"):
            greedy_inducing(K, x, 4, first=first)
    bad = np.array(x)
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="infs or NaNs"):
        greedy_inducing(K, bad, 4)
    with pytest.raises(ValueError, match="invalid shape for x"):
        greedy_inducing(K, np.zeros((2, 2, 2)), 1)
    with pytest.raises(ValueError, match=r"x has 2 dimension\(s\), the kernel has 3 width\(s\)"):
        greedy_inducing(gp.GaussianARDKernel(1.0, [1.0, 2.0, 3.0]), x, 4)
    with pytest.raises(AssertionError, match="the library was touched"):          # (and a good call does reach it)
        greedy_inducing(K, x, 4)


def _K(case, rows, cols):
    x = case_data(case)[0]
    okind, op, xv = oracle_view(kind_of(case), case[4], x)
    xv = xv.reshape(x.shape[0], -1)
    return orc.kernel_matrix(okind, "K", xv[rows], xv[cols], op)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_restatement_is_a_pivoted_partial_cholesky(case):
    f = free(case)
    k0, n = k0_of(case), case[1]
    idx, R, count = f["index"], f["R"], f["count"]
    print("%s: %d picks, last pivot %.2e k(0), E32R %.2e k(0)" % (case[:4], count, f["pivot"][-1] / k0, E32R[case] / k0))
    assert count == FP64_PICKS[case]
    assert len(set(idx.tolist())) == count and f["trace"].shape == (count + 1,) and R.shape == (count, n)
    # R[:, index] is upper triangular (below the diagonal: the residual of a picked point, rounding) with the pivots' square
    # roots on its diagonal, and R^T R reproduces the picked columns K(x, z).  The periodic case goes on to pivots of
    # 1.8e-8 k(0), whose rows carry the rounding of the rows before them divided by sqrt(pivot)
    U = R[:, idx]
    rounding = 1e-7 if case[0] == "periodic" else 1e-10
    assert np.abs(np.tril(U, -1)).max(initial=0.0) <= rounding * np.sqrt(k0)
    np.testing.assert_allclose(np.diag(U), np.sqrt(f["pivot"]), rtol=0.0, atol=rounding * np.sqrt(k0))
    np.testing.assert_allclose(R.T @ U, _K(case, slice(None), idx), rtol=0.0, atol=rounding * k0)
    # the residual is the diagonal of K - R^T R; trace and pivot behave
    np.testing.assert_allclose(f["res"][-1], np.where(np.isin(np.arange(n), idx), 0.0, k0 - (R * R).sum(0)), rtol=0.0, atol=1e-12 * k0)
    assert np.all(np.diff(f["trace"]) < 0.0)
    assert np.all(np.diff(f["pivot"]) <= 0.0)
    assert abs(f["trace"][0] - n * k0) <= 1e-13 * n * k0 and f["pivot"][0] == k0
    assert np.all(f["pivot"] > f["tol"]) and f["tol"] == auto_tol(case, np.float64)
    if count < case[3]:
        assert f["res"][-1].max() <= f["tol"]


def test_edge_cases_of_the_restatement():
    assert free(FULL)["count"] == 40 and sorted(free(FULL)["index"].tolist()) == list(range(40))     # M = N: every point
    assert free(ONE)["count"] == 1 and free(ONE)["index"][0] == 0                                      # all tie: the smallest index
    assert free(TABLE[4])["count"] == 16                                                               # periodic: an early stop
    assert free(TABLE[3], np.float32)["count"] == 47 and free(TABLE[4], np.float32)["count"] == 9      # fp32 stops earlier
    x = case_data(DUP)[0]
    z = x[free(DUP)["index"]]
    assert len(np.unique(z, axis=0)) == 60 and len(np.unique(x, axis=0)) == 300                        # never both copies of a row
    f = greedy(FULL, first=17)
    assert f["index"][0] == 17 and f["count"] == 40
    assert greedy(FULL, tol=0.0)["count"] == 40


@pytest.mark.parametrize("case", WELL, ids=CASE_IDS[:3])
def test_trace_is_the_trace_term_and_greedy_beats_random_subsets(case):
    x = case_data(case)[0]
    f = free(case)
    assert f["pivot"][-1] > 1e-2 * k0_of(case)
    z = x[f["index"]]
    # trace[-1] = kff - tr X = -2 s^2 * (the trace term of the bound) at jitter 0
    np.testing.assert_allclose(f["trace"][-1], -2.0 * elbo_at(case, z, jitter=0.0)["terms"]["trace"], rtol=1e-9, atol=0.0)
    greedy_elbo = elbo_at(case, z)["elbo"]
    random_elbo = [elbo_at(case, gp.SparseGP.subset_inducing(x, case[3], seed))["elbo"] for seed in SEEDS]
    print("%s: elbo greedy %.2f, best of the random subsets %.2f" % (case[:4], greedy_elbo, max(random_elbo)))
    assert greedy_elbo > max(random_elbo) + 2.7
