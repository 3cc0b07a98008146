"""GPU tests of IterativeGP / gpx_cg_* (csrc/gpx_cg.hip) against the dense GP, numpy and the restatement of tests/_cg_helpers.py.

Every tolerance is derived: kappa = lambda_max / lambda_min of K + s^2 I from the oracle's matrix (problem D: the bound
(n k0 + s^2) / s^2), tol = sqrt(eps) the solver's relative residual, and a solve that stops at |r| <= tol |b| is within
kappa tol |x| of the solution.  The conditions on the problems that make maxiter = 200 ample are asserted on the CPU
(tests/test_cg_cpu.py)."""
import ctypes
import warnings

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from _cg_helpers import (EPS, MAXITER, M_TEST, easy_rhs, PROBLEMS, SMALL, TOL, data, kappa, kappa_precond, kernel_between, kxx, make_kernel, pcg,
                         reference, true_relres)

pytestmark = pytest.mark.gpu

ORACLE_VAR = dict(rtol=1e-7, atol=1e-10)      # tests/test_gpu_var.py: the dense variance against the oracle

_IGP, _DENSE = {}, {}


def igp(name, **kw):
    """A fresh IterativeGP on a problem of the table (rank and maxiter = 200 from it unless given)."""
    x, y, _ = data(name)
    args = dict(precond_rank=PROBLEMS[name][5], maxiter=MAXITER)
    args.update(kw)
    return gp.IterativeGP(make_kernel(name), x, y, PROBLEMS[name][4], **args)


def shared(name):
    """One IterativeGP per problem, solved once, for the tests that only read it."""
    if name not in _IGP:
        _IGP[name] = igp(name)
        _IGP[name].inv_Kxx_y
    return _IGP[name]


def dense(name):
    if name not in _DENSE:
        x, y, _ = data(name)
        _DENSE[name] = gp.GP(make_kernel(name), x, y, PROBLEMS[name][4])
    return _DENSE[name]


# ---- the preconditioner block alone ----
@pytest.mark.parametrize("name", SMALL)
def test_precond_apply_alone(name):
    """gpx_cg_precond_apply on 5 random vectors against numpy's (R^T R + s^2 I)^-1 V with R from greedy_inducing(factor=True):
    relative error at most n eps kappa(P); count equals greedy_inducing's."""
    x, y, _ = data(name)
    n, s, rank = PROBLEMS[name][1], PROBLEMS[name][4], PROBLEMS[name][5]
    _, info = gp.SparseGP.greedy_inducing(make_kernel(name), x, rank, return_info=True, factor=True)
    R = info["R"]
    g = igp(name)
    st = g._state()
    assert st.rank == info["count"] == R.shape[0]
    assert (st.rank < rank) == (name == "B")                          # B's selection stops at its tolerance: count < rank is no error
    V = np.random.RandomState(11).randn(5, n)
    out = np.empty_like(V)
    _lib.check(_lib.load().gpx_cg_precond_apply(st.handle, _lib.dptr(V), 5, _lib.dptr(out)))
    want = np.linalg.solve(R.T @ R + s * s * np.eye(n), V.T).T
    err = np.linalg.norm(out - want) / np.linalg.norm(want)
    bound = n * EPS * kappa_precond(R, s)
    print("%s precond apply: rel err %.3e bound %.3e (kappa(P) %.3e, rank %d)" % (name, err, bound, kappa_precond(R, s), st.rank))
    assert err <= bound


def test_precond_apply_rank_zero_is_the_identity():
    g = igp("B", precond_rank=0)
    V = np.random.RandomState(12).randn(2, PROBLEMS["B"][1])
    out = np.empty_like(V)
    _lib.check(_lib.load().gpx_cg_precond_apply(g._state().handle, _lib.dptr(V), 2, _lib.dptr(out)))
    assert np.array_equal(out, V) and g._state().rank == 0


# ---- the solution ----
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_solution_against_the_dense_gp(name):
    """|alpha - alpha_dense| <= 2 kappa tol |alpha| (the factor 2 covers the dense solve's own error)."""
    g = shared(name)
    alpha, info = g.inv_Kxx_y, g.solve_info
    want = dense(name).inv_Kxx_y
    err, bound = np.linalg.norm(alpha - want), 2.0 * kappa(name) * TOL * np.linalg.norm(want)
    print("%s: iterations %d relres %.3e rank %d |dalpha| %.3e bound %.3e" % (name, info["iterations"][0], info["relres"][0], info["rank"],
                                                                              err, bound))
    assert info["converged"][0] and 0 < info["iterations"][0] <= MAXITER and info["relres"][0] <= TOL * (1 + 4 * EPS)
    assert err <= bound


@pytest.mark.parametrize("name", SMALL)
def test_true_residual_and_iterations_against_the_restatement(name):
    """The true residual |y - (K + s^2 I) alpha| / |y| formed in numpy is within x 4 of the restatement's on the same problem (a
    different summation order), and the device needs at most the restatement's iterations + 2."""
    g, ref, y = shared(name), reference(name), data(name)[1]
    got = true_relres(ref["A"], g.inv_Kxx_y, y)
    its = int(g.solve_info["iterations"][0])
    print("%s: true residual device %.3e restatement %.3e; iterations device %d restatement %d" % (name, got, ref["true_relres"], its,
                                                                                                 ref["iterations"][0]))
    assert got <= 4.0 * ref["true_relres"]
    assert its <= ref["iterations"][0] + 2


def test_the_preconditioner_saves_iterations_on_A():
    g0 = igp("A", precond_rank=0)
    g0.inv_Kxx_y
    its0, its = int(g0.solve_info["iterations"][0]), int(shared("A").solve_info["iterations"][0])
    print("A: %d iterations with rank 0, %d with rank 64 (restatement: %d, %d)" % (its0, its, reference("A", 0)["iterations"][0],
                                                                               reference("A")["iterations"][0]))
    assert g0.solve_info["converged"][0] and g0.solve_info["rank"] == 0
    assert its0 > its
    assert its0 <= reference("A", 0)["iterations"][0] + 2


# ---- batches ----
def _rhs(S):
    """S right-hand sides on A: y, a zero column, then columns of K and random vectors in turn."""
    x, y, _ = data("A")
    rng = np.random.RandomState(21)
    rows = [y, np.zeros_like(y)]
    for i in range(2, 33):
        rows.append(kxx("A")[7 * i] if i % 2 == 0 else rng.randn(y.size))
    return np.ascontiguousarray(np.stack(rows)[:S]) if S > 1 else y[None, :].copy()


_SINGLE = {}


def _single(i):
    """Column i of _rhs(33) solved alone, once."""
    if i not in _SINGLE:
        _SINGLE[i] = shared("A").solve(_rhs(33)[i])
    return _SINGLE[i]


@pytest.mark.parametrize("S", [1, 3, 8, 9, 33])
def test_batches_agree_with_single_columns(S):
    """S = 1, 3, 8, 9, 33 cross the fused product's vector blocks and the 32-column grouping: every column agrees with its own
    single-column solve within 2 kappa tol |x|; the zero column is exactly 0 with 0 iterations, and nothing is a NaN."""
    B = _rhs(S)
    X, info = shared("A").solve(B)
    assert X.shape == B.shape and np.all(np.isfinite(X)) and np.all(np.isfinite(info["relres"]))
    assert info["converged"].all() and info["iterations"].shape == (S,)
    k = kappa("A")
    for i in range(S):
        one, one_info = _single(i)
        assert np.linalg.norm(X[i] - one) <= 2.0 * k * TOL * np.linalg.norm(one), i
        assert abs(int(info["iterations"][i]) - int(one_info["iterations"][0])) <= 2, i
    if S > 1:
        assert np.all(X[1] == 0.0) and info["iterations"][1] == 0 and info["relres"][1] == 0.0


def test_an_early_column_is_frozen_bitwise():
    """[easy, hard] and [easy] with the same maxiter and no preconditioner (so that the two differ by many iterations): the
    easy column is bitwise what it was at its crossing, at the restatement's iteration count within 2."""
    g = igp("A", precond_rank=0)
    y = data("A")[1]
    easy, hard = easy_rhs(), y
    ref = pcg(reference("A", 0)["A"], np.stack([easy, hard]), np.zeros((0, y.size)), PROBLEMS["A"][4])
    assert ref["iterations"][0] + 3 <= ref["iterations"][1]
    X2, info2 = g.solve(np.stack([easy, hard]))
    X1, info1 = g.solve(easy)
    print("easy %d hard %d (restatement %s)" % (info2["iterations"][0], info2["iterations"][1], list(ref["iterations"])))
    assert info2["converged"].all() and info2["iterations"][0] < info2["iterations"][1]
    assert info1["iterations"][0] == info2["iterations"][0] and abs(int(info1["iterations"][0]) - int(ref["iterations"][0])) <= 2
    assert np.array_equal(X1, X2[0])
    assert info1["relres"][0] == info2["relres"][0]
    g.maxiter = int(info2["iterations"][0])                           # the same batch, stopped at the easy column's crossing
    X3, info3 = g.solve(np.stack([easy, hard]))
    assert info3["converged"][0] and not info3["converged"][1] and np.array_equal(X3[0], X2[0]) and not np.array_equal(X3[1], X2[1])


# ---- maxiter = 2 ----
def test_maxiter_two_is_reported_not_raised():
    """converged is False and nothing raises; relres is the numpy residual of the returned iterate within x 4 of the
    restatement's drift between the recurrence and the true residual; inv_Kxx_y warns once."""
    g = igp("A", maxiter=2)
    ref, y = reference("A"), data("A")[1]
    two = pcg(ref["A"], y, ref["R"], PROBLEMS["A"][4], maxiter=2)
    X, info = g.solve(y)
    assert not info["converged"][0] and info["iterations"][0] == 2 and np.all(np.isfinite(X))
    true = true_relres(ref["A"], X, y)
    drift = abs(two["relres"][0] - true_relres(ref["A"], two["X"][0], y))
    print("maxiter 2: relres %.6e true %.6e gap %.3e (restatement %.6e, drift %.3e)" % (info["relres"][0], true, abs(info["relres"][0] - true),
                                                                                   two["relres"][0], drift))
    assert abs(info["relres"][0] - true) <= 4.0 * drift
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        a1 = g.inv_Kxx_y
        a2 = g.inv_Kxx_y
    mine = [w for w in seen if issubclass(w.category, RuntimeWarning) and "maxiter = 2" in str(w.message)]
    assert len(mine) == 1 and "relative residual" in str(mine[0].message)
    assert a1 is a2 and not g.solve_info["converged"][0] and np.array_equal(a1, X)


# ---- predictions ----
@pytest.mark.parametrize("name", SMALL)
def test_mean_and_var_against_the_dense_gp(name):
    """mean at m = 70 within |k_i| 2 kappa tol |alpha| per point; var (70 = 32 + 32 + 6: a ragged last group) within
    tol |k_i|^2 / s^2 plus the dense value's own tolerance; noise=True adds s^2."""
    g, ref = shared(name), dense(name)
    x, _, xo = data(name)
    s = PROBLEMS[name][4]
    knorm = np.linalg.norm(kernel_between(name, xo, x), axis=1)
    mean, want = g.mean(xo), ref.mean(xo)
    bound = knorm * 2.0 * kappa(name) * TOL * np.linalg.norm(ref.inv_Kxx_y)
    print("%s mean: worst err / bound %.3e" % (name, float(np.max(np.abs(mean - want) / bound))))
    assert mean.shape == (M_TEST,) and np.all(np.abs(mean - want) <= bound)
    var, vwant = g.var(xo), ref.var(xo)
    vbound = TOL * knorm ** 2 / (s * s) + ORACLE_VAR["rtol"] * np.abs(vwant) + ORACLE_VAR["atol"]
    print("%s var: worst err / bound %.3e" % (name, float(np.max(np.abs(var - vwant) / vbound))))
    assert var.shape == (M_TEST,) and np.all(np.abs(var - vwant) <= vbound)
    assert np.array_equal(g.var(xo, noise=True), var + s ** 2)
    pm, pv = g.predict(xo)
    assert np.array_equal(pm, mean) and np.array_equal(pv, var)


# ---- repeatability and invalidation ----
def test_repeatable_bits_and_invalidation():
    g = igp("C")
    x, y, _ = data("C")
    B = np.stack([y, kxx("C")[3], np.cos(y)])
    X1, i1 = g.solve(B)
    X2, i2 = g.solve(B)
    assert np.array_equal(X1, X2) and np.array_equal(i1["relres"], i2["relres"]) and np.array_equal(i1["iterations"], i2["iterations"])
    a = g.inv_Kxx_y.copy()
    other = igp("C")
    assert np.array_equal(other.inv_Kxx_y, a) and np.array_equal(other.solve(B)[0], X1)
    # changing only y keeps R: the selection's route counter does not move, the solution does
    _lib.route_reset()
    g.y = y + 1.0
    b = g.inv_Kxx_y.copy()
    assert _lib.route_count(_lib.ROUTE_SELECT_STEP) == 0 and _lib.route_count(_lib.ROUTE_CG_ITER) == g.solve_info["iterations"][0] > 0
    assert not np.array_equal(a, b)
    # changing s or a kernel parameter rebuilds the preconditioner and invalidates the solution
    for change in (lambda: setattr(g, "s", 0.5), lambda: g.set_param("h", 1.5)):
        _lib.route_reset()
        change()
        c = g.inv_Kxx_y.copy()
        assert _lib.route_count(_lib.ROUTE_SELECT_STEP) == g.solve_info["rank"] > 0
        assert not np.array_equal(b, c)
        b = c
    ref = gp.GP(g.K, x, y + 1.0, 0.5)
    assert np.linalg.norm(b - ref.inv_Kxx_y) <= 2.0 * np.linalg.cond(ref.Kxx) * TOL * np.linalg.norm(ref.inv_Kxx_y)
    t = g.timing()
    assert set(t) == {"precond", "product", "apply", "vector", "total", "read"} and t["total"] > 0 and t["product"] > 0 and t["precond"] > 0


# ---- nothing n x n ----
def test_device_memory_is_linear_in_n():
    """On D the handle's device bytes are at most 8 n (d + 2 rank + 5 * 32 + 64): far below the 8 n^2 = 1.2 GB of a factor."""
    g = shared("D")
    _, n, d, _, _, rank = PROBLEMS["D"]
    X, info = g.solve(np.stack([data("D")[1]] * 2 + [np.ones(n)] * 31))      # 33 columns: the full-width state block
    assert info["converged"].all() and np.array_equal(X[0], X[1])
    got, bound = g.device_bytes, 8 * n * (d + 2 * rank + 5 * 32 + 64)
    print("D: %d device bytes, bound %d, a factor %d" % (got, bound, 8 * n * n))
    assert 8 * n * (d + 2 * rank) < got <= bound < 8 * n * n // 20


# ---- errors at the C ABI ----
def test_errors_at_the_abi():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.gpx_cg_create(ctypes.byref(h), _lib.F32, _lib.KERNEL_GAUSSIAN, 16, 2) == _lib.ERR_UNSUPPORTED and not h
    assert "float64 only" in _lib.last_error()
    _lib.check(lib.gpx_cg_create(ctypes.byref(h), _lib.F64, _lib.KERNEL_GAUSSIAN, 16, 2))
    try:
        rng = np.random.RandomState(0)
        x, y, p = rng.rand(16, 2), rng.randn(16), np.array([1.0, 0.5])
        out, xo, count = np.empty(3), rng.rand(3, 2), ctypes.c_int64(0)
        _lib.check(lib.gpx_cg_set_data(h, _lib.dptr(x), _lib.dptr(y)))
        assert lib.gpx_cg_mean(h, _lib.dptr(p), _lib.dptr(xo), 3, _lib.dptr(out)) == _lib.ERR_ARG          # before any solve
        assert "no solution" in _lib.last_error()
        assert lib.gpx_cg_precond(h, _lib.dptr(p), 0.3, 17, 0.0, ctypes.byref(count)) == _lib.ERR_ARG      # rank > n
        assert "rank" in _lib.last_error()
        assert lib.gpx_cg_precond(h, _lib.dptr(p), 0.0, 4, 0.0, ctypes.byref(count)) == _lib.ERR_ARG       # s = 0
        iters, relres, X = ctypes.c_int(0), ctypes.c_double(0.0), np.empty(16)
        assert lib.gpx_cg_solve(h, _lib.dptr(p), 0.3, None, 1, TOL, 50, _lib.dptr(X), ctypes.byref(iters), ctypes.byref(relres)) == _lib.ERR_ARG
        assert "no preconditioner" in _lib.last_error()
        _lib.check(lib.gpx_cg_precond(h, _lib.dptr(p), 0.3, 16, 0.0, ctypes.byref(count)))                 # rank = n, tol 0
        assert 1 <= count.value <= 16
        _lib.check(lib.gpx_cg_solve(h, _lib.dptr(p), 0.3, None, 1, TOL, 50, _lib.dptr(X), ctypes.byref(iters), ctypes.byref(relres)))
        want = gp.GP(gp.GaussianKernel(1.0, 0.5), x, y, 0.3)
        assert 0 < iters.value <= 50 and relres.value <= TOL * (1 + 4 * EPS)
        assert np.linalg.norm(X - want.inv_Kxx_y) <= 2.0 * np.linalg.cond(want.Kxx) * TOL * np.linalg.norm(want.inv_Kxx_y)
        _lib.check(lib.gpx_cg_mean(h, _lib.dptr(p), _lib.dptr(xo), 3, _lib.dptr(out)))
        knorm = np.linalg.norm(gp.GaussianKernel(1.0, 0.5)(xo, x), axis=1)
        assert np.all(np.abs(out - want.mean(xo)) <= knorm * 2.0 * np.linalg.cond(want.Kxx) * TOL * np.linalg.norm(want.inv_Kxx_y))
        other = np.array([1.0, 0.6])
        assert lib.gpx_cg_mean(h, _lib.dptr(other), _lib.dptr(xo), 3, _lib.dptr(out)) == _lib.ERR_ARG      # other parameters
        assert "other parameters" in _lib.last_error()
        assert lib.gpx_cg_solve(h, _lib.dptr(other), 0.3, None, 1, TOL, 50, _lib.dptr(X), ctypes.byref(iters), ctypes.byref(relres)) == _lib.ERR_ARG
    finally:
        lib.gpx_cg_destroy(h)
    # a d beyond the fused product's range is refused at creation: the solver has no other product
    assert lib.gpx_cg_create(ctypes.byref(h), _lib.F64, _lib.KERNEL_GAUSSIAN, 16, 48) == _lib.ERR_UNSUPPORTED and not h
    assert "fused route" in _lib.last_error()
    _lib.check(lib.gpx_cg_create(ctypes.byref(h), _lib.F64, _lib.KERNEL_GAUSSIAN, 16, 47))
    lib.gpx_cg_destroy(h)


def test_the_fused_switch_sets_the_group_and_is_never_bypassed():
    """gpx_debug_kapply_fused_max lowers the group size (9 columns at 8: two groups, still the fused route); at 0 a solve is
    refused, never sent through the product route."""
    g, B = shared("A"), _rhs(9)
    want = g.solve(B)[0]
    assert _lib.kapply_fused_max(8) == -1
    try:
        _lib.route_reset()
        X, info = g.solve(B)
        assert info["converged"].all() and _lib.route_count(_lib.ROUTE_KAPPLY_GEMM) == 0 and _lib.route_count(_lib.ROUTE_KAPPLY_FUSED) > 0
        for i in range(9):
            assert np.linalg.norm(X[i] - want[i]) <= 2.0 * kappa("A") * TOL * np.linalg.norm(want[i])
        _lib.kapply_fused_max(0)
        with pytest.raises(NotImplementedError, match="switched off"):
            g.solve(B)
        assert _lib.route_count(_lib.ROUTE_KAPPLY_GEMM) == 0
    finally:
        _lib.kapply_fused_max(-1)
    assert np.array_equal(g.solve(B)[0], want)
