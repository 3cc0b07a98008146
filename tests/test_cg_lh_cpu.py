"""CPU tests of IterativeGP's marginal-likelihood estimate (no GPU): the numpy restatement of tests/_cg_lh_helpers.py -- PCG that
records its coefficients, and the Lanczos quadrature on them -- pinned against dense references, the conditions
tests/test_gpu_cg_lh.py relies on, the refusals that come before the library is touched, and the header and the bindings."""
import os
import re
from ctypes import POINTER, c_double, c_int, c_int64, c_uint64, c_void_p

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from gaussian_processes_amd.iterative import DEFAULT_PROBES, lanczos_quadrature
from conftest import ROOT
from _sample_helpers import randn_ref
from _cg_helpers import PROBLEMS, SMALL, TOL, data, kappa, reference
from _cg_lh_helpers import (Q_TOL, dense_grad, estimate, exact_probes, given_probes, grad_restated, logdet, logdet_precond, lowrank_sums,
                            pcg_record, precond_matrix, probe_terms, quadrature)

c_double_p, c_int_p = POINTER(c_double), POINTER(c_int)


# ---- 1. the restatement against the dense references ----
@pytest.mark.parametrize("name", SMALL)
def test_restated_quadrature_against_the_dense_logarithm(name):
    """Per probe, rho0 e1^T log(T) e1 of the restatement equals u^T log(P^-1/2 (K + s^2 I) P^-1/2) u within Q_TOL rho0 / 100 -- the
    rows of P^1/2 (rho0 = 1) and the 33 given Gaussian rows, at rank 0 and at the table's rank -- and with the exact-trace
    probes sqrt(n) P^1/2 (rho0 = n each) the estimate reproduces slogdet(K + s^2 I) within n Q_TOL / 100 (measured: a relative
    3e-14 or better on every problem)."""
    n, s = PROBLEMS[name][1], PROBLEMS[name][4]
    for rank in (0, PROBLEMS[name][5]):
        ref = reference(name, rank)
        for what, Z in (("rows of P^1/2", precond_matrix(name, rank)[1]), ("given", given_probes(name))):
            _, terms, rec = estimate(ref["A"], Z, ref["R"], s)
            want = probe_terms(name, rank, Z)
            unit = np.abs(terms - want) / rec["rho0"]
            print("%s rank %d %s: worst per-probe error %.3e per unit of rho0 (Q_TOL / 100 = %.3e), terms up to %.3e, %d iterations"
                  % (name, ref["R"].shape[0], what, unit.max(), Q_TOL[name] / 100.0, np.abs(want).max(), rec["its"]))
            assert (rec["iterations"] > 0).all() and (rec["relres"] <= TOL).all()
            assert np.all(unit <= Q_TOL[name] / 100.0)
        ld, terms, rec = estimate(ref["A"], exact_probes(name, rank), ref["R"], s)
        np.testing.assert_allclose(rec["rho0"], n, rtol=1e-10)
        print("%s rank %d exact trace: log det %.12f dense %.12f rel err %.3e" % (name, ref["R"].shape[0], ld, logdet(name),
                                                                               abs(ld - logdet(name)) / abs(logdet(name))))
        assert abs(ld - logdet(name)) <= n * Q_TOL[name] / 100.0


def test_quadrature_of_the_package_is_the_restatements():
    """iterative.lanczos_quadrature (scipy's tridiagonal eigensolver) against the helper's dense eigh on recorded coefficients,
    and the edge cases: no iteration is 0, one iteration is log(1 / alpha_0)."""
    ref = reference("B", 0)
    rec = pcg_record(ref["A"], given_probes("B")[:3], ref["R"], PROBLEMS["B"][4])
    for t in range(3):
        m = rec["iterations"][t]
        a, b = rec["alpha"][:m, t], rec["beta"][:m, t]
        assert abs(lanczos_quadrature(a, b) - quadrature(a, b)) <= 1e-12 * max(1.0, abs(quadrature(a, b)))
    assert lanczos_quadrature([], []) == 0.0 and quadrature([], []) == 0.0
    assert lanczos_quadrature([0.25], [0.0]) == np.log(4.0) == quadrature([0.25], [0.0])


def test_logdet_of_the_preconditioner():
    for name in SMALL:
        n, s = PROBLEMS[name][1], PROBLEMS[name][4]
        R = reference(name)["R"]
        want = np.linalg.slogdet(precond_matrix(name, PROBLEMS[name][5])[0])[1]
        assert abs(logdet_precond(R, s, n) - want) <= 1e-10 * abs(want)
    assert logdet_precond(np.zeros((0, 5)), 0.3, 5) == 0.0


@pytest.mark.parametrize("name", SMALL)
def test_restated_gradient_with_exact_probes_is_the_dense_gradient(name):
    """1/2 alpha^T dK alpha - 1/2 (1/T) sum_t w_t^T dK zt_t with the exact-trace probes at the table's rank equals the dense
    1/2 tr((alpha alpha^T - A^-1) dK) within 2 tol kappa of the sum of the terms' magnitudes: E[zt z^T] = I holds exactly for
    them, and the solves stop at tol."""
    rank = PROBLEMS[name][5]
    got = grad_restated(name, rank, exact_probes(name, rank))
    want, mag = dense_grad(name)
    bound = 2.0 * TOL * kappa(name) * mag
    print("%s: gradient %s dense %s worst err / bound %.3e" % (name, got, want, float(np.max(np.abs(got - want) / bound))))
    assert np.all(np.abs(got - want) <= bound)


def test_generated_probes_pass_on_A_with_the_chosen_seed():
    """The condition of the GPU test of generated probes, on the restatement with the generator's restatement: with 32 probes
    z = g1 R + s g2 (g2 = randn_ref(stream 4), g1 = randn_ref(stream 5)) of seed 0 the estimate of log det lies within 5
    standard errors of the dense value, at rank 0 and at rank 64, and the preconditioner lowers the standard error."""
    n, s = PROBLEMS["A"][1], PROBLEMS["A"][4]
    stderr = {}
    for rank in (0, PROBLEMS["A"][5]):
        ref = reference("A", rank)
        R = ref["R"]
        Z = randn_ref(DEFAULT_PROBES, n, 0, stream=4)
        if R.shape[0]:
            Z = randn_ref(DEFAULT_PROBES, R.shape[0], 0, stream=5) @ R + s * Z
        ld, terms, _ = estimate(ref["A"], Z, R, s)
        stderr[rank] = terms.std(ddof=1) / np.sqrt(DEFAULT_PROBES)
        print("A rank %d seed 0: log det %.6f dense %.6f stderr %.4f: %.2f standard errors" % (R.shape[0], ld, logdet("A"), stderr[rank],
                                                                                           abs(ld - logdet("A")) / stderr[rank]))
        assert abs(ld - logdet("A")) <= 5.0 * stderr[rank]
    assert stderr[PROBLEMS["A"][5]] < stderr[0]


def test_lowrank_sums_reference_is_consistent():
    """The dense reference of the reduction: with U = V = alpha its slots give the quadratic half of the dense gradient."""
    kind, n, _, params, s, _ = PROBLEMS["B"]
    x, y, _ = data("B")
    alpha = np.linalg.solve(reference("B", 0)["A"], y)
    sums, mags = lowrank_sums(kind, params, x, alpha[None, :], alpha[None, :])
    from _cg_lh_helpers import kernel_derivatives
    J = kernel_derivatives(kind, params, x)
    for p in range(3):
        assert abs(sums[p] - alpha @ J[p] @ alpha) <= 1e-12 * mags[p]
    assert abs(sums[3] - alpha @ alpha) <= 1e-12 * mags[3] and np.all(mags >= np.abs(sums))


# ---- 2. refusals before the library ----
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def _make(**kw):
    rng = np.random.RandomState(0)
    return gp.IterativeGP(gp.GaussianKernel(1.0, 1.0), rng.randn(10, 3), rng.randn(10), 0.5, **kw)


def test_the_names_say_estimate(no_library):
    g = _make()
    assert not hasattr(g, "log_lh") and not hasattr(g, "dloglh_dtheta")
    for name in ("log_lh_estimate", "log_lh_and_grad", "probes", "optimize"):
        assert callable(getattr(g, name))
    assert "estimate" in gp.IterativeGP.log_lh_estimate.__doc__ and "expectation" in gp.IterativeGP.optimize.__doc__.lower()
    assert DEFAULT_PROBES == 32


@pytest.mark.parametrize("probes", [0, -1, 2.5, True, "x", np.zeros(10), np.zeros((2, 9)), np.zeros((0, 10)), np.zeros((2, 10, 1))],
                         ids=["zero", "negative", "float", "bool", "str", "1d", "short_rows", "no_rows", "3d"])
@pytest.mark.parametrize("method", ["log_lh_estimate", "log_lh_and_grad", "optimize"])
def test_bad_probes_are_refused_before_the_library(no_library, method, probes):
    with pytest.raises(ValueError, match="probes"):
        getattr(_make(), method)(probes=probes)


def test_non_finite_probes_and_bad_seeds_are_refused_before_the_library(no_library):
    Z = np.ones((2, 10))
    Z[1, 3] = np.inf
    with pytest.raises(ValueError, match="infs or NaNs"):
        _make().log_lh_estimate(probes=Z)
    for seed in (-1, 2 ** 64, 1.5, True, None):
        with pytest.raises(ValueError, match="seed"):
            _make().log_lh_estimate(seed=seed)
        with pytest.raises(ValueError, match="seed"):
            _make().probes(3, seed=seed)
    for T in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="T"):
            _make().probes(T)
    with pytest.raises(ValueError, match="bounds"):
        _make().optimize(bounds=[(None, None)])


# ---- 3. header, library and bindings ----
def test_lh_symbols_are_declared_exported_and_bound():
    want = {
        "gpx_cg_probes": (c_int, [c_void_p, c_int64, c_uint64, c_double_p]),
        "gpx_cg_lh": (c_int, [c_void_p, c_double_p, c_double, c_double_p, c_int64, c_uint64, c_double, c_int64, c_int, c_double_p, c_int_p,
                              c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
        "gpx_d_lowrank_reduce": (c_int, [c_int, c_int, c_void_p, c_int64, c_int, c_double_p, c_void_p, c_void_p, c_int64, c_int64, c_double_p,
                                         c_void_p]),
    }
    hdr = open(os.path.join(ROOT, "include", "gpx.h")).read()
    assert "streams 4 and 5" in hdr                                   # the list of the generator's streams that are taken
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, (res, args) in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), "include/gpx.h does not declare %s" % name
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name][0] is res
        assert list(_lib._SIGNATURES[name][1]) == args, name
        assert getattr(lib, name).argtypes == args
    for macro, value in (("GPX_PROF_LOWRANK", 24), ("GPX_ROUTE_LOWRANK", 28)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr), macro
    assert (_lib.PROF_LOWRANK, _lib.ROUTE_LOWRANK) == (24, 28)
    csrc = os.path.join(ROOT, "gaussian_processes_amd", "csrc")
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    assert "gpx_lrgrad.hip" in srcs
    # the history pointer is null in every solve but the estimate's: one call site passes a record
    cg = open(os.path.join(csrc, "gpx_cg.hip")).read()
    assert len(re.findall(r"cg_solve_group\([^;]*&rec\)", cg)) == 1
    # float32 and bad arguments are refused before a device is asked for
    p, out = np.array([1.0, 1.0]), np.zeros(4)
    one = c_void_p(16)
    assert lib.gpx_d_lowrank_reduce(_lib.F32, _lib.KERNEL_GAUSSIAN, one, 4, 1, _lib.dptr(p), one, one, 4, 1, _lib.dptr(out), None) == _lib.ERR_UNSUPPORTED
    assert "float64 only" in _lib.last_error()
    assert lib.gpx_d_lowrank_reduce(_lib.F64, _lib.KERNEL_GAUSSIAN, one, 4, 1, _lib.dptr(p), one, one, 4, 0, _lib.dptr(out), None) == _lib.ERR_ARG
    assert "T >= 1" in _lib.last_error()
    assert lib.gpx_d_lowrank_reduce(_lib.F64, _lib.KERNEL_GAUSSIAN, one, 4, 1, _lib.dptr(p), None, one, 4, 1, _lib.dptr(out), None) == _lib.ERR_ARG
    assert "NULL pointer" in _lib.last_error()
