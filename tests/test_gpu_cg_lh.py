"""GPU tests of IterativeGP's marginal-likelihood estimate: the low-rank tile reduction alone (gpx_d_lowrank_reduce,
csrc/gpx_lrgrad.hip), the probes (gpx_cg_probes), the pass (gpx_cg_lh) and the facade (log_lh_estimate, log_lh_and_grad,
optimize) against numpy, the dense GP and the restatement of tests/_cg_lh_helpers.py.

Bounds: Q_TOL rho0 per probe term (100 x the restatement's own error, tests/_cg_lh_helpers.py; tests/test_cg_lh_cpu.py pins the
restatement a factor 100 inside); 2 tol kappa of the terms' magnitudes for a gradient whose solves stop at tol = sqrt(eps); a
rounding bound with its term count written out for the reduction alone.

The exact-trace probes are sqrt(n) I (rank 0) and sqrt(n) P^1/2: rows whose second moment Z^T Z / T is exactly P, which the
estimator's (1/T) sum_t asks of given probes.  (The rows of I alone have the second moment I / n: their mean is tr / n.)"""
import ctypes
import warnings

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib, mlii
from _ard_helpers import iso_params
from _extend_helpers import DeviceBuffers
from _sample_helpers import randn_ref
from _cg_helpers import MAXITER, PROBLEMS, SMALL, TOL, data, kappa, make_kernel, reference
from _cg_lh_helpers import (OPT_SHORTFALL, Q_TOL, T_GIVEN, dense_grad, given_probes, log_of_whitened, logdet, lowrank_sums, sqrt_pair,
                            terms_of)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_KID = {"gaussian": _lib.KERNEL_GAUSSIAN, "periodic": _lib.KERNEL_PERIODIC, "ard": _lib.KERNEL_GAUSSIAN_ARD}
_IGP, _DENSE, _FACTOR = {}, {}, {}


def igp(name, **kw):
    x, y, _ = data(name)
    args = dict(precond_rank=PROBLEMS[name][5], maxiter=MAXITER)
    args.update(kw)
    return gp.IterativeGP(make_kernel(name), x, y, PROBLEMS[name][4], **args)


def shared(name, rank):
    """One IterativeGP per (problem, rank) for the tests that only read it."""
    if (name, rank) not in _IGP:
        _IGP[name, rank] = igp(name, precond_rank=rank)
    return _IGP[name, rank]


def dense(name):
    if name not in _DENSE:
        x, y, _ = data(name)
        _DENSE[name] = gp.GP(make_kernel(name), x, y, PROBLEMS[name][4])
    return _DENSE[name]


def device_factor(name, rank):
    """(R of the device's selection, P, P^1/2, P^-1/2, log(P^-1/2 (K + s^2 I) P^-1/2)), once per (problem, rank)."""
    if (name, rank) not in _FACTOR:
        n, s = PROBLEMS[name][1], PROBLEMS[name][4]
        R = np.zeros((0, n))
        if rank > 0:
            R = gp.SparseGP.greedy_inducing(make_kernel(name), data(name)[0], rank, return_info=True, factor=True)[1]["R"]
        P, Ph, Pmh = sqrt_pair(R, s, n)
        A = reference(name, 0)["A"]
        _FACTOR[name, rank] = (R, P, Ph, Pmh, log_of_whitened(A, Pmh))
    return _FACTOR[name, rank]


# ---- 1. the reduction alone ----
_NS, _TS = (1, 63, 64, 65, 129, 257), (1, 2, 32, 33, 70)
_FAMILIES = [("gaussian", 1), ("gaussian", 3), ("gaussian", 32), ("periodic", 1), ("ard", 2), ("ard", 5), ("ard", 47)]


def _family_case(kind, d, n, seed):
    """(points as the kernel sees them, its parameters, the family's own (kind, params, x) for the reference)."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(0.0, 1.0, (n, d))
    if kind == "gaussian":
        params = (1.3, 0.4 * np.sqrt(d))
        return x, np.array(params), (kind, params, x)
    if kind == "periodic":
        params = (1.0, 0.8, 0.3)
        return x, np.array(params), (kind, params, x.ravel())
    w = np.linspace(0.3, 1.6, d) * np.sqrt(d)
    params = (1.2,) + tuple(w)
    return np.ascontiguousarray(x / w), np.array(iso_params(1.2, w)), (kind, params, x)


def _reduce(dev, kid, dx, n, d, prm, dU, dV, ld, T, width, dtype=_lib.F64):
    out = np.full(width, np.nan)
    rc = dev.lib.gpx_d_lowrank_reduce(dtype, kid, dx, n, d, _lib.dptr(prm), dU, dV, ld, T, _lib.dptr(out), None)
    return rc, out


@pytest.mark.parametrize("kind,d", _FAMILIES, ids=["%s-d%d" % f for f in _FAMILIES])
def test_lowrank_reduce_alone(kind, d):
    """gpx_d_lowrank_reduce against numpy on c = U^T V for n in {1, 63, 64, 65, 129, 257} x T in {1, 2, 32, 33, 70} (d = 47 is the
    largest the handle takes), U and V with NaN in their pads beyond n, twice for the bits, one route hit per 32 rows.
    Bound per slot: terms u sum |U|^T |V| |dk_p| with
        terms = 2 T (the dot, here and in numpy) + 2 (d + 3) (1 + emax) (the distance's d + 1 roundings and the scaled exponent's,
                amplified by the exponent's size emax = max |log(k / k0)| <= 706 into the exponential; both sides)
                + 16 (the exponential, the derivative's polynomial and constants, the product with c; the periodic family's sine
                and cosine) + 16 + 8 + ceil(n / 64)^2 (a thread's 16 entries, the block sum's 6 + 2 levels, one partial per
                workgroup added in order) + 2 log2(n^2) (numpy's pairwise sum)."""
    width = d + 2 if kind == "ard" else 4
    worst = 0.0
    with DeviceBuffers() as dev:
        for n in _NS:
            xk, prm, (rkind, rparams, rx) = _family_case(kind, d, n, seed=n)
            dx = dev.put(xk)
            d2 = ((xk[:, None, :] - xk[None, :, :]) ** 2).sum(axis=2)
            emax = 2.0 / prm[1] ** 2 if kind == "periodic" else min(706.0, float(d2.max()) * 0.5 / prm[1] ** 2)
            for T in _TS:
                rng = np.random.RandomState(1000 * n + T)
                ld = n + 3
                Uh, Vh = np.full((T, ld), np.nan), np.full((T, ld), np.nan)
                Uh[:, :n], Vh[:, :n] = rng.randn(T, n), rng.randn(T, n)
                dU, dV = dev.put(Uh), dev.put(Vh)
                _lib.route_reset()
                rc, got = _reduce(dev, _KID[kind], dx, n, d, prm, dU, dV, ld, T, width)
                _lib.check(rc)
                assert _lib.route_count(_lib.ROUTE_LOWRANK) == (T + 31) // 32
                rc, again = _reduce(dev, _KID[kind], dx, n, d, prm, dU, dV, ld, T, width)
                _lib.check(rc)
                assert np.array_equal(got, again) and np.all(np.isfinite(got)), (n, T, got)
                ref, mag = lowrank_sums(rkind, rparams, rx, Uh[:, :n], Vh[:, :n])
                terms = 2 * T + 2 * (d + 3) * (1.0 + emax) + 16 + 16 + 8 + ((n + 63) // 64) ** 2 + 2 * np.log2(n * n + 1.0)
                bound = terms * U * mag
                ratio = float(np.max(np.abs(got - ref) / np.maximum(bound, 1e-300)))
                worst = max(worst, ratio)
                assert np.all(np.abs(got - ref) <= bound), (n, T, got, ref, bound)
                if kind == "gaussian":
                    assert got[2] == 0.0
    print("lowrank_reduce %s d=%d: worst err / bound %.3e" % (kind, d, worst))


# ---- 2. per-probe quadrature with given probes ----
@pytest.mark.parametrize("ranked", [False, True], ids=["rank0", "table_rank"])
@pytest.mark.parametrize("name", SMALL)
def test_per_probe_quadrature_with_given_probes(name, ranked):
    """33 fixed Gaussian rows from numpy: every per-probe term rho0 e1^T log(T) e1 within Q_TOL rho0 of the dense
    u^T log(P^-1/2 (K + s^2 I) P^-1/2) u, with P from the device's own selection."""
    rank = PROBLEMS[name][5] if ranked else 0
    g = shared(name, rank)
    Z = given_probes(name)
    R, P, _, Pmh, logM = device_factor(name, rank)
    value, info = g.log_lh_estimate(probes=Z, return_info=True)
    want = terms_of(Z, Pmh, logM)
    rho0 = np.einsum("ti,ti->t", Z @ Pmh, Z @ Pmh)
    err = np.abs(info["quad"] - want)
    print("%s rank %d: worst per-probe err / (Q_TOL rho0) %.3e (err %.3e), iterations up to %d" % (name, info["rank"], float(np.max(err / (Q_TOL[name] * rho0))),
                                                                                             float(err.max()), int(info["iterations"].max())))
    assert info["quad"].shape == (T_GIVEN,) and info["converged"].all() and info["rank"] == R.shape[0]
    assert np.all(err <= Q_TOL[name] * rho0)
    assert np.isfinite(value) and abs(info["logdet"] - (info["logdet_precond"] + info["quad"].mean())) <= 1e-12 * abs(info["logdet"])
    if rank:
        want_p = np.linalg.slogdet(P)[1]
        assert abs(info["logdet_precond"] - want_p) <= 1e-10 * abs(want_p)
    else:
        assert info["logdet_precond"] == 0.0


# ---- 3. the exact trace ----
@pytest.mark.parametrize("ranked", [False, True], ids=["rank0", "table_rank"])
@pytest.mark.parametrize("name", SMALL)
def test_exact_trace_value_and_gradient_against_the_dense_gp(name, ranked):
    """With the exact-trace probes (sqrt(n) I at rank 0; sqrt(n) P^1/2 from greedy_inducing's R with the preconditioner)
    log_lh_estimate equals GP.log_lh within n Q_TOL / 2 (every term carries rho0 = n; the log determinant enters halved) plus
    the fit term's CG error tol |y| |alpha| / 2 (y . (alpha - alpha*) = r . alpha*, |r| <= tol |y|) plus the dense value's own
    1e-10 relative (smoke()'s tolerance for it); and the gradient equals GP.dloglh_dtheta within 2 tol kappa of the sum of its
    terms' magnitudes.  GP.log_lh keeps the reference's clamp (-inf once log det < MIN: A and C); there the dense value is formed
    from the dense GP's own factor and solution, -1/2 y . alpha - sum log diag(Lxx) - n/2 log 2 pi, without the clamp."""
    n = PROBLEMS[name][1]
    rank = PROBLEMS[name][5] if ranked else 0
    g, ref = shared(name, rank), dense(name)
    Z = np.sqrt(n) * device_factor(name, rank)[2]
    value, grad = g.log_lh_and_grad(probes=Z)
    _, info = g.log_lh_estimate(probes=Z, return_info=True)
    y = data(name)[1]
    dense_lh = float(ref.log_lh)
    if not np.isfinite(dense_lh):
        assert logdet(name) < _lib.MIN_LOG                            # the clamp, not a failed fit
        dense_lh = float(-0.5 * y @ ref.inv_Kxx_y - np.log(np.diag(ref.Lxx)).sum() - 0.5 * n * np.log(2.0 * np.pi))
    bound = 0.5 * n * Q_TOL[name] + 0.5 * TOL * np.linalg.norm(y) * np.linalg.norm(ref.inv_Kxx_y) + 1e-10 * abs(dense_lh)
    print("%s rank %d: estimate %.10f dense %.10f err %.3e bound %.3e; log det %.10f numpy %.10f" % (name, info["rank"], value, dense_lh,
                                                                                                   abs(value - dense_lh), bound, info["logdet"], logdet(name)))
    assert info["converged"].all()
    assert abs(value - dense_lh) <= bound
    assert abs(info["logdet"] - logdet(name)) <= n * Q_TOL[name]
    want, mag = np.asarray(ref.dloglh_dtheta), dense_grad(name)[1]
    gbound = 2.0 * TOL * kappa(name) * mag
    print("%s rank %d gradient: %s dense %s worst err / bound %.3e" % (name, info["rank"], grad, want, float(np.max(np.abs(grad - want) / gbound))))
    assert grad.shape == want.shape == (g.params.size,)
    assert np.all(np.abs(grad - want) <= gbound)


# ---- 4. the device's probes ----
def test_device_probes():
    """Rank 0: z = g2 = randn_ref(stream 4) to the generator's tolerance.  Rank 64: z - g1 R - s g2 at rounding level,
    (k + 2) u (|g1| |R| + s |g2|) plus the generator's tolerance through either factor.  A prefix in T; the same bits twice."""
    n, s = PROBLEMS["A"][1], PROBLEMS["A"][4]
    seed, T = 7, 33
    g0 = shared("A", 0)
    z0 = g0.probes(T, seed)
    assert z0.shape == (T, n) and float(np.abs(z0 - randn_ref(T, n, seed, stream=4)).max()) <= 1e-13
    g = shared("A", PROBLEMS["A"][5])
    z = g.probes(T, seed)
    R = device_factor("A", PROBLEMS["A"][5])[0]
    g1, g2 = randn_ref(T, R.shape[0], seed, stream=5), randn_ref(T, n, seed, stream=4)
    bound = (R.shape[0] + 2) * U * (np.abs(g1) @ np.abs(R) + s * np.abs(g2)) + 1e-13 * (np.abs(R).sum(axis=0) + s)
    err = np.abs(z - g1 @ R - s * g2)
    print("probes rank %d: worst err / bound %.3e" % (R.shape[0], float((err / bound).max())))
    assert np.all(err <= bound)
    assert np.array_equal(g.probes(5, seed), z[:5]) and np.array_equal(g.probes(T, seed), z) and np.array_equal(g0.probes(32, seed), z0[:32])
    assert not np.array_equal(g.probes(5, seed + 1), z[:5])


# ---- 5. generated probes ----
def test_generated_probes_on_A_lie_within_five_standard_errors():
    """32 device probes of seed 0 (the seed tests/test_cg_lh_cpu.py checks on the restatement): the estimate of log det lies
    within 5 stderr of numpy's, at rank 0 and at rank 64, and the preconditioner lowers the stderr."""
    stderr = {}
    for rank in (0, PROBLEMS["A"][5]):
        value, info = shared("A", rank).log_lh_estimate(probes=32, seed=0, return_info=True)
        stderr[rank] = info["stderr"]
        print("A rank %d: log det %.6f numpy %.6f stderr %.4f (%.2f standard errors)" % (info["rank"], info["logdet"], logdet("A"), info["stderr"],
                                                                                       abs(info["logdet"] - logdet("A")) / info["stderr"]))
        assert info["quad"].shape == (32,) and info["converged"].all()
        assert abs(info["logdet"] - logdet("A")) <= 5.0 * info["stderr"]
        assert value == shared("A", rank).log_lh_estimate()              # probes=None is 32 of seed 0
        assert abs(value - (info["fit"] - 0.5 * info["logdet"] - 0.5 * PROBLEMS["A"][1] * np.log(2.0 * np.pi))) <= 1e-12 * abs(value)
    assert stderr[PROBLEMS["A"][5]] < stderr[0]


# ---- 6. bookkeeping ----
def test_repeatable_bits_memoisation_and_invalidation():
    g, other = igp("C"), igp("C")
    x, y, _ = data("C")
    v1, g1 = g.log_lh_and_grad(probes=5, seed=3)
    v2, g2 = other.log_lh_and_grad(probes=5, seed=3)
    assert v1 == v2 and np.array_equal(g1, g2)
    _lib.route_reset()
    assert g.log_lh_estimate(probes=5, seed=3) == v1 and np.array_equal(g.log_lh_and_grad(probes=5, seed=3)[1], g1)      # memoized
    assert _lib.route_count(_lib.ROUTE_CG_ITER) == 0 and _lib.route_count(_lib.ROUTE_LOWRANK) == 0
    assert g.log_lh_estimate(probes=5, seed=4) != v1 and _lib.route_count(_lib.ROUTE_LOWRANK) == 0                       # no gradient asked
    g.log_lh_and_grad(probes=33, seed=3)
    assert _lib.route_count(_lib.ROUTE_LOWRANK) == 3                  # 32 + 1 probes, then alpha
    for change in (lambda: setattr(g, "s", 0.5), lambda: g.set_param("h", 1.5), lambda: setattr(g, "y", y + 1.0), lambda: setattr(g, "x", x * 1.01)):
        before = g.log_lh_estimate(probes=5, seed=3)
        _lib.route_reset()
        change()
        after = g.log_lh_estimate(probes=5, seed=3)
        assert after != before and _lib.route_count(_lib.ROUTE_CG_ITER) > 0
    fresh = gp.IterativeGP(g.K, g.x, g.y, g.s, precond_rank=PROBLEMS["C"][5], maxiter=MAXITER)
    assert fresh.log_lh_estimate(probes=5, seed=3) == after


def test_maxiter_two_warns_and_returns():
    g = igp("A", maxiter=2)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        value, info = g.log_lh_estimate(probes=3, return_info=True)
    mine = [w for w in seen if issubclass(w.category, RuntimeWarning) and "maxiter = 2" in str(w.message)]
    assert any("probe solves" in str(w.message) for w in mine)
    assert np.isfinite(value) and not info["converged"].any() and list(info["iterations"]) == [2, 2, 2] and np.all(np.isfinite(info["quad"]))


def test_a_handle_that_never_asks_keeps_its_device_bytes():
    """The estimate's block is allocated by the first estimate: before it the handle reports the bytes of a handle that only
    solves (the state block's layout is untouched), after it at least 32 more rows of n doubles."""
    n = PROBLEMS["B"][1]
    g, never = igp("B"), igp("B")
    g.inv_Kxx_y, never.inv_Kxx_y
    before = g.device_bytes
    assert before == never.device_bytes
    g.solve(np.ones((33, n)))
    never.solve(np.ones((33, n)))
    full = g.device_bytes
    assert full == never.device_bytes
    g.log_lh_estimate(probes=2)
    assert never.device_bytes == full and g.device_bytes >= full + 8 * 32 * n
    grown = g.device_bytes
    g.log_lh_estimate(probes=40, seed=1)
    assert g.device_bytes == grown                                    # grow-only, and already at its full width


def test_errors_at_the_abi():
    lib = _lib.load()
    g = igp("B")
    st = g._state()
    n = PROBLEMS["B"][1]
    p = np.ascontiguousarray(g.K.params)
    rho0, relres, coef, scal, sums, grad = np.empty(2), np.empty(2), np.empty((2, MAXITER, 2)), np.empty(2), np.empty(4), np.empty(4)
    iters = (ctypes.c_int * 2)()

    def call(params=p, s=float(g.s), T=2, rho=rho0, want_grad=1, sm=sums):
        return lib.gpx_cg_lh(st.handle, None if params is None else _lib.dptr(params), s, None, T, 0, TOL, MAXITER, want_grad,
                             None if rho is None else _lib.dptr(rho), iters, _lib.dptr(relres), _lib.dptr(coef), _lib.dptr(scal),
                             None if sm is None else _lib.dptr(sm), _lib.dptr(grad))
    assert call(T=0) == _lib.ERR_ARG and "T >= 1" in _lib.last_error()
    assert call(rho=None) == _lib.ERR_ARG and "NULL argument" in _lib.last_error()
    assert call(sm=None) == _lib.ERR_ARG and "NULL argument" in _lib.last_error()
    assert call(params=None) == _lib.ERR_ARG and "NULL argument" in _lib.last_error()
    assert call(s=0.7) == _lib.ERR_ARG and "no preconditioner" in _lib.last_error()
    assert call(sm=None, want_grad=0) == _lib.OK
    assert call() == _lib.OK and np.all(np.isfinite(grad))
    assert lib.gpx_cg_probes(st.handle, 0, 0, None) == _lib.ERR_ARG and "T >= 1" in _lib.last_error()
    assert lib.gpx_cg_probes(None, 1, 0, None) == _lib.ERR_ARG and "handle is NULL" in _lib.last_error()
    assert lib.gpx_cg_probes(st.handle, 3, 0, None) == _lib.OK
    with DeviceBuffers() as dev:
        d = dev.put(np.zeros((4, 4)))
        out = np.zeros(4)
        prm = np.array([1.0, 1.0])
        assert lib.gpx_d_lowrank_reduce(_lib.F32, _lib.KERNEL_GAUSSIAN, d, 4, 1, _lib.dptr(prm), d, d, 4, 1, _lib.dptr(out), None) == _lib.ERR_UNSUPPORTED
        assert "float64 only" in _lib.last_error()
        assert lib.gpx_d_lowrank_reduce(_lib.F64, _lib.KERNEL_GAUSSIAN, d, 4, 1, _lib.dptr(prm), d, None, 4, 1, _lib.dptr(out), None) == _lib.ERR_ARG
        assert lib.gpx_d_lowrank_reduce(_lib.F64, _lib.KERNEL_GAUSSIAN, d, 4, 1, _lib.dptr(prm), d, d, 3, 1, _lib.dptr(out), None) == _lib.ERR_ARG
        assert lib.gpx_d_lowrank_reduce(_lib.F64, _lib.KERNEL_PERIODIC, d, 4, 2, _lib.dptr(prm), d, d, 4, 1, _lib.dptr(out), None) == _lib.ERR_ARG


# ---- 7. optimize ----
def test_optimize_reaches_the_dense_optimum():
    """A 200 x 2 Gaussian problem, the exact-trace probes sqrt(n) I at rank 0, from a perturbed start, against mlii.optimize from
    the same start with the same maxiter and bounds: the dense log_lh at the parameters IterativeGP.optimize reaches falls short
    of the dense optimum's by at most OPT_SHORTFALL (tests/_cg_lh_helpers.py: 10 x the shortfall measured on the device) plus the
    two dense values' own 1e-10 relative, and whatever that number, optimize ends above its start and leaves the object at the best parameters it evaluated."""
    rng = np.random.RandomState(77)
    n = 200
    x = rng.uniform(0.0, 1.0, (n, 2))
    y = np.sin(4.0 * x[:, 0]) + np.cos(3.0 * x[:, 1]) + 0.1 * rng.randn(n)
    theta0 = np.array([0.5, 0.15, 0.3])
    maxiter = 30
    bounds = [(t / 100.0, t * 100.0) for t in theta0]

    def dense_lh(theta):                                             # without the reference's clamp, as mlii.optimize follows it
        ref = gp.GP(gp.GaussianKernel(theta[0], theta[1]), x, y, theta[2])
        return float(-0.5 * y @ ref.inv_Kxx_y - np.log(np.diag(ref.Lxx)).sum() - 0.5 * n * np.log(2.0 * np.pi))
    g = gp.IterativeGP(gp.GaussianKernel(theta0[0], theta0[1]), x, y, theta0[2], precond_rank=0, maxiter=n)
    Z = np.sqrt(n) * np.eye(n)
    first = g.log_lh_estimate(probes=Z)
    res = g.optimize(maxiter=maxiter, bounds=bounds, probes=Z)
    best = mlii.optimize(x, y, theta0[None, :], maxiter=maxiter)
    start, reached, optimum = dense_lh(theta0), dense_lh(res["params"]), float(best["log_lh"][0])
    print("optimize: start %.6f reached %.6f (estimate %.6f, %d evaluations) mlii %.6f: shortfall %.3e (allowed %.3e); params %s mlii %s"
          % (start, reached, res["log_lh_estimate"], res["evaluations"], optimum, optimum - reached, OPT_SHORTFALL, res["params"], best["theta"][0]))
    assert set(res) >= {"params", "log_lh_estimate", "evaluations"} and res["evaluations"] >= 2
    assert np.array_equal(res["params"], g.params)
    assert reached > start and res["log_lh_estimate"] > first
    assert optimum - reached <= OPT_SHORTFALL + 2e-10 * abs(optimum)
