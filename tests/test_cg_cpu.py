"""CPU tests of IterativeGP / gpx_cg_* (no GPU): the numpy restatement of the algorithm (tests/_cg_helpers.py) and the conditions
on the problem table that tests/test_gpu_cg.py relies on, the refusals that come before the library is touched, and the header
and the binding of the new entry points."""
import copy
import os
import pickle
import re
from ctypes import POINTER, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from conftest import ROOT
from test_dist_gp_cpu import _PythonRBF
from _cg_helpers import (MAXITER, easy_rhs, PROBLEMS, SMALL, TOL, data, kappa, kxx, make_kernel, partial_cholesky, pcg, reference, select_tol,
                         true_relres, woodbury)

c_double_p, c_int_p = POINTER(c_double), POINTER(c_int)


# ---- 1. the restatement, and the conditions on the table ----
@pytest.mark.parametrize("name", SMALL)
def test_restatement_converges_within_the_gpu_tests_maxiter(name):
    """A - C reach tol = sqrt(eps) in at most 200 iterations with the preconditioner: the GPU tests' maxiter = 200 cannot hide a
    failure.  And the solution agrees with numpy.linalg.solve within kappa tol |alpha|."""
    ref = reference(name)
    y = data(name)[1]
    print("%s: rank %d iterations %d relres %.3e true %.3e kappa %.3e" % (name, ref["R"].shape[0], ref["iterations"][0], ref["relres"][0],
                                                                         ref["true_relres"], kappa(name)))
    assert ref["frozen"][0] and 0 < ref["iterations"][0] <= MAXITER
    assert ref["relres"][0] <= TOL
    alpha = np.linalg.solve(ref["A"], y)
    assert np.linalg.norm(ref["X"][0] - alpha) <= kappa(name) * TOL * np.linalg.norm(alpha)


def test_the_preconditioner_halves_the_iterations_on_A():
    """Rank 0 needs at least twice the iterations of rank 64 on A: the gap the GPU test of the preconditioner needs."""
    with_p, without = reference("A")["iterations"][0], reference("A", 0)["iterations"][0]
    print("A: %d iterations with rank 64, %d with none" % (with_p, without))
    assert without >= 2 * with_p


@pytest.mark.parametrize("name", SMALL)
def test_restated_partial_cholesky_and_woodbury(name):
    """R^T R reproduces the picked columns of K, the picks are distinct, and the Woodbury apply inverts P = R^T R + s^2 I."""
    s = PROBLEMS[name][4]
    ref = reference(name)
    R, index, K = ref["R"], ref["index"], kxx(name)
    assert len(set(index.tolist())) == len(index) == R.shape[0] <= PROBLEMS[name][5]
    assert np.abs((R.T @ R)[:, index] - K[:, index]).max() <= 1e-12 * K.max()
    V = np.random.RandomState(2).randn(3, K.shape[0])
    P = R.T @ R + s * s * np.eye(K.shape[0])
    assert np.abs(woodbury(R, s, V) @ P - V).max() <= 1e-9 * np.abs(V).max()
    if R.shape[0] < PROBLEMS[name][5]:                                # the selection stopped at its tolerance
        resid = np.diag(K) - (R * R).sum(axis=0)
        assert resid.max() <= select_tol(name) * (1 + 1e-9)


def test_restated_freezing_and_zero_column():
    """A zero right-hand side is frozen from the start (x = 0, 0 iterations, relres 0, no NaN); a column that converged early
    is bitwise what its own single-column solve gives, whatever its companions do."""
    s = PROBLEMS["A"][4]
    A, y, K = reference("A", 0)["A"], data("A")[1], kxx("A")
    none = np.zeros((0, A.shape[0]))
    B = np.stack([easy_rhs(), y, np.zeros_like(y)])
    rec = pcg(A, B, none, s)
    assert np.all(np.isfinite(rec["X"])) and np.all(rec["X"][2] == 0.0)
    assert rec["iterations"][2] == 0 and rec["relres"][2] == 0.0
    assert rec["iterations"][0] + 3 <= rec["iterations"][1]           # an easy column and a hard one
    rng = np.random.RandomState(0)
    for _ in range(3):                                                # the easy column's crossing is sharp: rounding does not move it
        assert pcg(A, B[0] * (1.0 + 1e-15 * rng.randn(B.shape[1])), none, s)["iterations"][0] == rec["iterations"][0]
    alone = pcg(A, B[:1], none, s)
    assert alone["iterations"][0] == rec["iterations"][0] and np.array_equal(alone["X"][0], rec["X"][0])
    two = pcg(A, B, none, s, maxiter=2)
    assert not two["frozen"][:2].any() and list(two["iterations"]) == [2, 2, 0]
    assert abs(two["relres"][1] - true_relres(A, two["X"][1], y)) <= 1e-12


# ---- 2. refusals before the library ----
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def _make(**kw):
    rng = np.random.RandomState(0)
    args = dict(K=gp.GaussianKernel(1.0, 1.0), x=rng.randn(10, 3), y=rng.randn(10), s=0.5)
    args.update(kw)
    return gp.IterativeGP(args.pop("K"), args.pop("x"), args.pop("y"), args.pop("s"), **args)


def test_constructor_defaults(no_library):
    g = _make()
    assert g.tol == float(np.sqrt(np.finfo(np.float64).eps)) and g.maxiter == 10 and g.precond_rank == 0
    assert _make(precond_rank=10).precond_rank == 10 and _make(maxiter=7, tol=1e-3).maxiter == 7
    assert list(g.params) == [1.0, 1.0, 0.5]
    for missing in ("log_lh", "cov", "sample", "dloglh_dtheta"):
        assert not hasattr(g, missing)
        assert missing in gp.IterativeGP.__doc__ or missing == "dloglh_dtheta"
    for f in (copy.copy, copy.deepcopy, pickle.dumps):
        with pytest.raises(NotImplementedError, match="not copied or pickled"):
            f(g)


@pytest.mark.parametrize("kw,exc,what", [
    (dict(s=0.0), ValueError, "s"), (dict(s=-1.0), ValueError, "s"), (dict(s=np.inf), ValueError, "s"),
    (dict(K=_PythonRBF(1.3, 0.9)), NotImplementedError, "plugin kernels are not supported"),
    (dict(dtype="float32"), NotImplementedError, "float64 only"),
    (dict(precond_rank=-1), ValueError, "precond_rank"), (dict(precond_rank=11), ValueError, "precond_rank"),
    (dict(precond_rank=2.0), ValueError, "precond_rank"), (dict(precond_rank=True), ValueError, "precond_rank"),
    (dict(tol=0.0), ValueError, "tol"), (dict(tol=-1e-3), ValueError, "tol"), (dict(tol=1.0), ValueError, "tol"),
    (dict(tol=np.nan), ValueError, "tol"), (dict(tol="x"), ValueError, "tol"), (dict(tol=True), ValueError, "tol"),
    (dict(maxiter=0), ValueError, "maxiter"), (dict(maxiter=1.5), ValueError, "maxiter"),
    (dict(y=np.zeros(9)), ValueError, "y"), (dict(x=np.zeros((10, 3, 1))), ValueError, "x"),
], ids=["s_zero", "s_negative", "s_inf", "plugin", "float32", "rank_negative", "rank_beyond_n", "rank_float", "rank_bool", "tol_zero",
        "tol_negative", "tol_one", "tol_nan", "tol_str", "tol_bool", "maxiter_zero", "maxiter_float", "y_shape", "x_shape"])
def test_constructor_refusals_before_the_library(no_library, kw, exc, what):
    with pytest.raises(exc, match=what):
        _make(**kw)


@pytest.mark.parametrize("B", [np.zeros(9), np.zeros((2, 9)), np.zeros((2, 10, 1)), np.zeros((0, 10)), np.float64(1.0)],
                         ids=["short", "short_rows", "3d", "no_rows", "scalar"])
def test_solve_refuses_bad_shapes_before_the_library(no_library, B):
    with pytest.raises(ValueError, match="B"):
        _make().solve(B)


def test_solve_refuses_non_finite_before_the_library(no_library):
    B = np.zeros(10)
    B[3] = np.nan
    with pytest.raises(ValueError, match="infs or NaNs"):
        _make().solve(B)


@pytest.mark.parametrize("xo", [np.zeros((2, 4)), np.zeros(2), np.zeros((2, 3, 1))], ids=["wrong_d", "xo_1d", "xo_3d"])
@pytest.mark.parametrize("method", ["mean", "var", "predict"])
def test_predictions_refuse_bad_xo_before_the_library(no_library, method, xo):
    with pytest.raises(ValueError, match="xo"):
        getattr(_make(), method)(xo)


def test_ard_widths_must_match_x(no_library):
    g = gp.IterativeGP(gp.GaussianARDKernel(1.0, [1.0, 2.0]), np.zeros((5, 3)), np.zeros(5), s=1.0)
    with pytest.raises(ValueError, match="width"):
        g.inv_Kxx_y


# ---- 3. header, library and bindings ----
def test_cg_symbols_are_declared_exported_and_bound():
    want = {
        "gpx_cg_create": (c_int, [POINTER(c_void_p), c_int, c_int, c_int64, c_int]),
        "gpx_cg_destroy": (c_int, [c_void_p]),
        "gpx_cg_set_data": (c_int, [c_void_p, c_double_p, c_double_p]),
        "gpx_cg_precond": (c_int, [c_void_p, c_double_p, c_double, c_int64, c_double, POINTER(c_int64)]),
        "gpx_cg_precond_apply": (c_int, [c_void_p, c_double_p, c_int64, c_double_p]),
        "gpx_cg_solve": (c_int, [c_void_p, c_double_p, c_double, c_double_p, c_int64, c_double, c_int64, c_double_p, c_int_p, c_double_p]),
        "gpx_cg_mean": (c_int, [c_void_p, c_double_p, c_double_p, c_int64, c_double_p]),
        "gpx_cg_var": (c_int, [c_void_p, c_double_p, c_double, c_double_p, c_int64, c_double, c_int64, c_double_p, c_double_p]),
        "gpx_cg_last_timing": (c_int, [c_void_p, POINTER(c_float)]),
        "gpx_cg_device_bytes": (c_int, [c_void_p, POINTER(c_size_t)]),
    }
    hdr = open(os.path.join(ROOT, "include", "gpx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, (res, args) in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), "include/gpx.h does not declare %s" % name
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name][0] is res
        assert list(_lib._SIGNATURES[name][1]) == args, name
        assert getattr(lib, name).argtypes == args                    # (resolves it in the built library)
    for macro, value in (("GPX_PROF_CG", 23), ("GPX_ROUTE_CG_ITER", 27)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr), macro
    assert (_lib.PROF_CG, _lib.ROUTE_CG_ITER) == (23, 27)
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(ROOT, "gaussian_processes_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "gpx_cg.hip" in srcs
    assert gp.IterativeGP is gp.iterative.IterativeGP and "IterativeGP" in gp.__all__


def test_the_selection_has_a_device_pointer_entry_and_no_new_switch():
    """The preconditioner runs the selection on the handle's resident x through an internal entry of gpx_select.hip declared in
    gpx_gp_internal.h; the solver brings no environment switch."""
    csrc = os.path.join(ROOT, "gaussian_processes_amd", "csrc")
    internal = open(os.path.join(csrc, "gpx_gp_internal.h")).read()
    assert re.search(r"\bint select_on_device\(", internal) and re.search(r"\bsize_t select_block_bytes\(", internal)
    assert not re.findall(r'"(GPX_[A-Z0-9_]+)"', open(os.path.join(csrc, "gpx_cg.hip")).read())


def test_a_rank_beyond_a_smaller_x_is_refused_before_the_library(no_library):
    g = _make(precond_rank=8)
    g.x, g.y = np.zeros((5, 3)), np.zeros(5)                          # (y is checked against the new x when it is assigned)
    with pytest.raises(ValueError, match="precond_rank"):
        g.inv_Kxx_y
