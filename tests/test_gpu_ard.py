"""GPU tests of the Gaussian ARD family (GPX_KERNEL_GAUSSIAN_ARD, gp.GaussianARDKernel): the reduction to the isotropic
kernel at equal widths, general widths against the oracle on pre-scaled inputs, the device gradient, the lock-step batch,
ML-II, checkpoints and the refusals.

Tolerances are the project's own for the same quantity, restated from tests/test_gpu_parity.py with the same constants:
KTOL for kernel matrices of one formula, the golden records' C_COND * cond(Kxx) * eps * scale bound, rtol 1e-10 (log_lh),
1e-8 / 1e-11 (alpha, mean), ORACLE_TOL (cov, var, predict; tests/test_gpu_var.py) against the oracle; fp32: log_lh 1e-4,
alpha 2e-3 / 2e-4 max, mean 1e-3 / 1e-3, cov and var 1e-2 / 5e-3, the gradient 2e-2 / 1e-1 -- the fp32 lines of that file.
An fp32 kernel matrix has no line there: its squared distance carries up to d eps32 ~ 2e-6 relative (d = 32), multiplied by
an exponent of up to ~50 where entries still matter: rtol 1e-4, and 1e-6 max|K| absolute for the entries beyond.
Batch against single handle: rtol 1e-10, the bound of tests/test_gpu_round6.py for the Gaussian family's gradient."""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib, mlii
from oracle import gp_oracle as orc
from conftest import load_golden
from _ard_helpers import ard_K, ard_grad, iso_params

pytestmark = pytest.mark.gpu

KTOL = dict(rtol=1e-13, atol=1e-300)       # tests/test_gpu_parity.py
C_COND = 16.0                              # tests/test_gpu_parity.py: |got - ref| <= C_COND * cond(Kxx) * eps * scale
_EPS = np.finfo(np.float64).eps
ORACLE_TOL = {"float64": dict(rtol=1e-7, atol=1e-10), "float32": dict(rtol=1e-2, atol=5e-3)}
F32_GRAD = dict(rtol=2e-2, atol=1e-1)      # tests/test_gpu_parity.py, the fp32 gradient against the oracle


def _nclose(got, ref, tol, scale, what):
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))))
    bound = tol * max(float(scale), 1e-300)
    print("%s: err %.3e bound %.3e (%.3f of it)" % (what, err, bound, err / bound))
    assert err <= bound, "%s: |got - ref| = %.3e exceeds C_COND cond eps scale = %.3e" % (what, err, bound)


def _data(N, d, m=48):
    """SURVEY 8(d) inputs on [-1, 1]^d: widths in [0.3, 3] then leave the kernel matrix far from diagonal."""
    X, y, Xo = orc.synth_inputs(N, d, m)
    return X / 10.0, y, Xo / 10.0


def _widths(d, seed=7):
    return np.random.RandomState(seed).uniform(0.3, 3.0, d)


# ------------------------------------------------------------------ 1. reduction to the isotropic kernel --
@pytest.mark.parametrize("w", [0.5, 2.0])
@pytest.mark.parametrize("d", [1, 3, 32])
def test_equal_power_of_two_widths_are_the_isotropic_kernel(d, w):
    N, h, s = 600, 1.3, 0.7
    X, y, Xo = _data(N, d)
    if d == 1:
        X, Xo = X.ravel(), Xo.ravel()
    ka, ki = gp.GaussianARDKernel(h, np.full(d, w)), gp.GaussianKernel(h, w)
    np.testing.assert_allclose(ka(Xo, X), ki(Xo, X), **KTOL)
    ga, gi = gp.GP(ka, X, y, s=s), gp.GP(ki, X, y, s=s)
    Kxx = gi.Kxx
    np.testing.assert_allclose(ga.Kxx, Kxx, **KTOL)
    np.testing.assert_allclose(ga.log_lh, gi.log_lh, rtol=1e-10)
    tol = C_COND * float(np.linalg.cond(Kxx)) * _EPS
    alpha, Kinv, Kxox = gi.inv_Kxx_y, gi.inv_Kxx, ki(Xo, X)
    amax, rs = float(np.abs(alpha).max()), float(np.abs(Kxox).sum(1).max())
    cscale = np.abs(ki(Xo, Xo)).max() + rs * rs * np.abs(Kinv).max()
    _nclose(ga.inv_Kxx_y, alpha, tol, amax, "inv_Kxx_y")
    _nclose(ga.mean(Xo), gi.mean(Xo), tol, rs * amax, "mean")
    _nclose(ga.var(Xo), gi.var(Xo), tol, cscale, "var")
    _nclose(ga.cov(Xo), gi.cov(Xo), tol, cscale, "cov")
    np.testing.assert_allclose(ka.diag(Xo), ki.diag(Xo), rtol=1e-14)
    # the gradient: h and s components are the isotropic ones, the width components sum to its w component
    aabs = np.abs(alpha)
    J = orc.jacobian("gaussian", X, X, np.array([h, w]))
    dK = [J[0], J[1], np.eye(N) * 2 * s]
    sc = [0.5 * (float(aabs @ np.abs(m_) @ aabs) + float((np.abs(Kinv) * np.abs(m_)).sum())) for m_ in dK]
    got, ref = ga.dloglh_dtheta, gi.dloglh_dtheta
    assert got.shape == (d + 2,)
    _nclose(got[0], ref[0], tol, sc[0], "dloglh/dh")
    _nclose(got[1:-1].sum(), ref[1], tol, sc[1], "sum_k dloglh/dw_k")
    _nclose(got[-1], ref[2], tol, sc[2], "dloglh/ds")
    np.testing.assert_allclose(ga.dlh_dtheta, ga.lh * got, rtol=1e-15)


def test_a_golden_record_as_d_1():
    """One record of tests/golden/gp_small.npz (outputs of the real reference) through the ARD family with one width."""
    npz = load_golden("gp_small.npz")
    rec = {k[len("rand03__"):]: npz[k] for k in npz.files if k.startswith("rand03__")}
    (h, w), s = rec["params"][:-1], rec["params"][-1]
    x, y, xo = rec["x"], rec["y"], rec["xo"]
    g = gp.GP(gp.GaussianARDKernel(h, [w]), x, y, s=s)
    K, Kinv, alpha = rec["Kxx"], rec["inv_Kxx"], rec["inv_Kxx_y"]
    tol = C_COND * float(np.linalg.cond(K)) * _EPS
    np.testing.assert_allclose(g.Kxx, K, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(g.Kxox(xo), rec["Kxox"], rtol=1e-12, atol=1e-300)
    amax, aabs = float(np.abs(alpha).max()), np.abs(alpha)
    n = x.shape[0]
    _nclose(g.inv_Kxx_y, alpha, tol, amax, "inv_Kxx_y")
    llh_scale = 0.5 * float(np.abs(y) @ aabs) + float(np.abs(np.log(np.diag(rec["Lxx"]))).sum()) + 0.5 * n * np.log(2 * np.pi)
    _nclose(g.log_lh, rec["log_lh"], tol, llh_scale, "log_lh")
    rs = float(np.abs(rec["Kxox"]).sum(1).max())
    cscale = np.abs(rec["Kxoxo"]).max() + rs * rs * np.abs(Kinv).max()
    _nclose(g.mean(xo), rec["mean"], tol, rs * amax, "mean")
    _nclose(g.cov(xo), rec["cov"], tol, cscale, "cov")
    _nclose(g.var(xo), np.diag(rec["cov"]), tol, cscale, "var")
    J = orc.jacobian("gaussian", x, x, np.array([h, w]))
    dK = [J[0], J[1], np.eye(n) * 2 * s]
    for i in range(3):
        sc = float(aabs @ np.abs(dK[i]) @ aabs) + float((np.abs(Kinv) * np.abs(dK[i])).sum())
        _nclose(g.dloglh_dtheta[i], rec["dloglh_dtheta"][i], tol, 0.5 * sc, "dloglh_dtheta[%d]" % i)


# ------------------------------------------------------------------ 2. general widths against the oracle --
_ORACLE = {}


def _oracle_case(d, N):
    if (d, N) not in _ORACLE:
        X, y, Xo = _data(N, d)
        h, w, s = 1.3, _widths(d), 0.7
        o = orc.OracleGP("gaussian", iso_params(h, w), X / w, y, s)
        xo_s = Xo / w
        ref = dict(Kxx=o.Kxx, log_lh=float(o.log_lh), alpha=o.inv_Kxx_y, mean=o.mean(xo_s), cov=o.cov(xo_s))
        _ORACLE.clear()                                           # (one n x n oracle at a time in host memory)
        _ORACLE[(d, N)] = (X, y, Xo, h, w, s, ref)
    return _ORACLE[(d, N)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("d", [3, 8, 32])
@pytest.mark.parametrize("N", [1000, 4200, 8192])
def test_general_widths_against_the_oracle_on_scaled_inputs(N, d, dtype):
    X, y, Xo, h, w, s, ref = _oracle_case(d, N)
    g = gp.GP(gp.GaussianARDKernel(h, w), X, y, s=s, dtype=dtype)
    f64 = dtype == "float64"
    _lib.route_reset()
    np.testing.assert_allclose(g.log_lh, ref["log_lh"], rtol=1e-10 if f64 else 1e-4)
    mean, var, cov = g.mean(Xo), g.var(Xo), g.cov(Xo)
    assert (_lib.route_count(_lib.ROUTE_TRSM_OPS) > 0) == (N == 8192)       # the operator route and the 64-wide one
    pm, pv = g.predict(Xo)
    if f64:
        np.testing.assert_allclose(g.Kxx, ref["Kxx"], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(g.inv_Kxx_y, ref["alpha"], rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(mean, ref["mean"], rtol=1e-8, atol=1e-11)
    else:
        np.testing.assert_allclose(g.Kxx, ref["Kxx"], rtol=1e-4, atol=1e-6 * np.abs(ref["Kxx"]).max())
        np.testing.assert_allclose(g.inv_Kxx_y, ref["alpha"], rtol=2e-3, atol=2e-4 * np.abs(ref["alpha"]).max())
        np.testing.assert_allclose(mean, ref["mean"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(cov, ref["cov"], **ORACLE_TOL[dtype])
    np.testing.assert_allclose(var, np.diag(ref["cov"]), **ORACLE_TOL[dtype])
    np.testing.assert_allclose(pm, ref["mean"], **(dict(rtol=1e-8, atol=1e-11) if f64 else dict(rtol=1e-3, atol=1e-3)))
    np.testing.assert_allclose(pv, np.diag(ref["cov"]), **ORACLE_TOL[dtype])
    if N == 1000 and f64:
        np.testing.assert_allclose(g.K(Xo, X), ard_K(Xo, X, h, w), rtol=1e-12, atol=1e-300)


def test_scale_points_is_numpy_division_bit_for_bit():
    lib = _lib.load()
    rs = np.random.RandomState(5)
    n, d = 1037, 13
    x, w = rs.randn(n, d), rs.uniform(0.3, 3.0, d)
    for dt, npdt in ((_lib.F64, np.float64), (_lib.F32, np.float32)):
        xs = np.ascontiguousarray(x, dtype=npdt)
        nbytes = xs.nbytes
        src, dst = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(lib.gpx_malloc(ctypes.byref(src), nbytes))
        _lib.check(lib.gpx_malloc(ctypes.byref(dst), nbytes))
        try:
            _lib.check(lib.gpx_memcpy_h2d(src, xs.ctypes.data_as(ctypes.c_void_p), nbytes, None))
            _lib.check(lib.gpx_d_scale_points(dt, src, n, d, _lib.dptr(w), dst, None))
            _lib.check(lib.gpx_d_scale_points(dt, src, n, d, _lib.dptr(w), src, None))          # in place
            a, b = np.empty_like(xs), np.empty_like(xs)
            _lib.check(lib.gpx_memcpy_d2h(a.ctypes.data_as(ctypes.c_void_p), dst, nbytes, None))
            _lib.check(lib.gpx_memcpy_d2h(b.ctypes.data_as(ctypes.c_void_p), src, nbytes, None))
            _lib.check(lib.gpx_device_sync())
        finally:
            lib.gpx_free(src); lib.gpx_free(dst)
        np.testing.assert_array_equal(a, xs / w.astype(npdt))
        np.testing.assert_array_equal(b, a)
    assert lib.gpx_d_scale_points(_lib.F64, None, 4, 65, _lib.dptr(np.ones(65)), None, None) == _lib.ERR_ARG


# ------------------------------------------------------------------ 3. the gradient --
GRAD_CASES = [(1000, 3), (1000, 12), (1000, 32), (1000, 40), (2048, 8)]       # d: every accumulator count the kernel is built for


@pytest.mark.parametrize("N,d", GRAD_CASES)
def test_gradient_against_the_closed_form_from_the_oracle(N, d):
    """GP.dloglh_dtheta against tests/_ard_helpers.ard_grad evaluated from the oracle's inv_Kxx and inv_Kxx_y, within the
    bound tests/test_gpu_parity.py::_check_gp_record applies to dloglh_dtheta, the scale formed from |dK/dtheta| of this
    family; fp32 at the fp32 gradient line of that file; two calls give identical bits."""
    X, y, _ = _data(N, d)
    h, w, s = 1.3, _widths(d), 0.7
    o = orc.OracleGP("gaussian", iso_params(h, w), X / w, y, s)
    ref, scale = ard_grad(X, h, w, s, o.inv_Kxx, o.inv_Kxx_y)
    tol = C_COND * float(np.linalg.cond(o.Kxx)) * _EPS
    g = gp.GP(gp.GaussianARDKernel(h, w), X, y, s=s)
    got = np.array(g.dloglh_dtheta)
    assert got.shape == (d + 2,)
    for i in range(d + 2):
        _nclose(got[i], ref[i], tol, 0.5 * scale[i], "dloglh_dtheta[%d]" % i)
    del g.dloglh_dtheta
    again = np.array(g.dloglh_dtheta)
    assert again.tobytes() == got.tobytes()
    g2 = gp.GP(gp.GaussianARDKernel(h, w), X, y, s=s)
    assert np.array(g2.dloglh_dtheta).tobytes() == got.tobytes()
    g32 = gp.GP(gp.GaussianARDKernel(h, w), X, y, s=s, dtype="float32")
    np.testing.assert_allclose(g32.dloglh_dtheta, ref, **F32_GRAD)


def test_gradient_central_differences_of_the_device_log_lh():
    N, d = 700, 5
    X, y, _ = _data(N, d)
    theta = np.concatenate([[1.3], _widths(d), [0.7]])
    g = gp.GP(gp.GaussianARDKernel(theta[0], theta[1:-1]), X, y, s=theta[-1])
    grad = np.array(g.dloglh_dtheta)
    fd = np.empty(d + 2)
    for i in range(d + 2):
        v = []
        for sgn in (-1.0, 1.0):
            t = theta.copy(); t[i] *= 1.0 + sgn * 1e-5
            g.params = t
            v.append(float(g.log_lh))
        fd[i] = (v[1] - v[0]) / (2e-5 * theta[i])
    np.testing.assert_allclose(grad, fd, rtol=2e-5, atol=1e-6 * np.abs(grad).max())


def test_gradient_of_a_fit_that_is_not_positive_definite_is_nan():
    X, y, _ = _data(1350, 2)
    g = gp.GP(gp.GaussianARDKernel(1.0, [1e4, 1e4]), X, y, s=0.0)
    assert g.log_lh == -np.inf
    got = g.dloglh_dtheta
    assert got.shape == (4,) and np.isnan(got).all()
    assert np.isnan(g.dlh_dtheta).all()


# ------------------------------------------------------------------ 4. the lock-step batch --
def test_batch_rows_equal_the_single_handle():
    N, d = 2048, 8
    X, y, _ = _data(N, d)
    rs = np.random.RandomState(11)
    th = np.column_stack([rs.uniform(0.5, 2, 8), rs.uniform(0.3, 3.0, (8, d)), rs.uniform(0.5, 1.5, 8)])
    th[2, 4] = 0.0                                                # a width below EPS: the reference's ValueError
    th[5, 1:-1] = 1e4; th[5, -1] = 0.0                            # rank deficient: not positive definite
    with mlii.BatchEvaluator(X, y, kernel="gaussian_ard") as ev:
        val = ev(th)
        val2, grad = ev.value_and_grad(th)
        with pytest.raises(ValueError):
            ev(th[:, :3])
    np.testing.assert_array_equal(val, val2)
    assert grad.shape == (8, d + 2)
    assert np.isnan(val[2]) and np.isnan(grad[2]).all()
    assert val[5] == -np.inf and np.isnan(grad[5]).all()
    for i in (0, 1, 3, 4, 6, 7):
        g = gp.GP(gp.GaussianARDKernel(th[i, 0], th[i, 1:-1]), X, y, s=th[i, -1])
        np.testing.assert_allclose(val[i], g.log_lh, rtol=1e-10)
        np.testing.assert_allclose(grad[i], g.dloglh_dtheta, rtol=1e-10)
    np.testing.assert_array_equal(mlii.log_lh_batch(X, y, th, kernel="gaussian_ard"), val)
    np.testing.assert_allclose(mlii.log_lh_batch(X, y, th[:2], kernel="gaussian_ard", batched=False), val[:2], rtol=1e-10)


def test_batch_in_chunks_and_fp32(monkeypatch):
    N, d = 1536, 5
    X, y, _ = _data(N, d)
    rs = np.random.RandomState(12)
    th = np.column_stack([rs.uniform(0.5, 2, 7), rs.uniform(0.3, 3.0, (7, d)), rs.uniform(0.8, 1.5, 7)])
    with mlii.BatchEvaluator(X, y, kernel="gaussian_ard") as ev:
        monkeypatch.setenv("GPX_BATCH_MAX", "3")
        v3, g3 = ev.value_and_grad(th, clamp=False)
        monkeypatch.delenv("GPX_BATCH_MAX", raising=False)
        v1, g1 = ev.value_and_grad(th, clamp=False)
    np.testing.assert_array_equal(v1, v3)
    np.testing.assert_array_equal(g1, g3)
    with mlii.BatchEvaluator(X, y, kernel="gaussian_ard", dtype="float32") as e32:
        v32, g32 = e32.value_and_grad(th, clamp=False)
    np.testing.assert_allclose(v32, v1, rtol=1e-4)                # tests/test_gpu_round6.py, fp32 against fp64
    np.testing.assert_allclose(g32, g1, rtol=5e-3, atol=5e-3 * np.abs(g1).max())


# ------------------------------------------------------------------ 5. ML-II finds the relevant inputs --
def test_the_optimiser_finds_the_relevant_inputs():
    rng = np.random.default_rng(0)
    n, d = 400, 6
    X = rng.uniform(-1, 1, (n, d))
    y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 + 0.05 * rng.standard_normal(n)
    y = y - y.mean()
    th0 = np.exp(np.random.default_rng(1).uniform(-1, 1, (4, d + 2)))
    bounds = np.tile([np.exp(-5.0), np.exp(5.0)], (d + 2, 1))
    res = mlii.optimize(X, y, th0, kernel="gaussian_ard", bounds=bounds, maxiter=100)
    w = res["theta"][res["best"], 1:-1]
    print("best restart: theta", res["theta"][res["best"]], "log_lh", res["log_lh"], "nit", res["nit"])
    assert (res["log_lh"] >= res["log_lh0"]).all()
    assert w[2:].min() >= 10.0 * w[:2].max()


# ------------------------------------------------------------------ 6. checkpoints --
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_checkpoint_restores_the_kernel_and_its_widths(tmp_path, dtype):
    N, d = 700, 6
    X, y, Xo = _data(N, d)
    h, w, s = 1.3, _widths(d), 0.7
    g = gp.GP(gp.GaussianARDKernel(h, w), X, y, s=s, dtype=dtype)
    llh, mean, var = g.log_lh, g.mean(Xo), g.var(Xo)
    path = tmp_path / "ard.gpx"
    g.save_fitted(path)
    r = gp.GP.load_fitted(path)
    assert type(r.K) is gp.GaussianARDKernel
    np.testing.assert_array_equal(r.K.params, g.K.params)
    np.testing.assert_array_equal(r.params, g.params)
    np.testing.assert_array_equal(r.x, X if dtype == "float64" else X.astype(np.float32).astype(np.float64))
    assert r.log_lh == llh
    assert r.mean(Xo).tobytes() == mean.tobytes()
    assert r.var(Xo).tobytes() == var.tobytes()
    lib = _lib.load()
    p3, full, cnt = np.zeros(3), np.zeros(1 + _lib.ARD_MAX_D), ctypes.c_int(0)
    _lib.check(lib.gpx_gp_describe(r._dev.handle, None, None, None, None, _lib.dptr(p3), None))
    assert p3[0] == h and np.isnan(p3[1:]).all()
    _lib.check(lib.gpx_gp_get_params(r._dev.handle, _lib.dptr(full), full.size, ctypes.byref(cnt)))
    assert cnt.value == d + 1
    np.testing.assert_array_equal(full[:d + 1], g.K.params)
    # a file of the isotropic family still loads (and holds no widths: header + x + y + alpha + the factor)
    gi = gp.GP(gp.GaussianKernel(h, 0.9), X, y, s=s, dtype=dtype)
    lli = gi.log_lh
    pi = tmp_path / "iso.gpx"
    gi.save_fitted(pi)
    ri = gp.GP.load_fitted(pi)
    assert type(ri.K) is gp.GaussianKernel and ri.log_lh == lli
    np.testing.assert_array_equal(ri.K.params, [h, 0.9])
    assert path.stat().st_size == pi.stat().st_size + 8 * d


# ------------------------------------------------------------------ 7. refusals --
def test_refusals():
    X, y, Xo = _data(300, 4)
    k = gp.GaussianARDKernel(1.3, _widths(4))
    g = gp.GP(k, X, y, s=0.7)
    g.log_lh
    with pytest.raises(NotImplementedError):
        g.d2lh_dtheta2
    with pytest.raises(NotImplementedError):
        g.d2loglh_dtheta2
    with pytest.raises(NotImplementedError):
        g.dm_dtheta(Xo)
    with pytest.raises(NotImplementedError):
        gp.DistributedGP(k, X, y, s=0.7)
    lib = _lib.load()
    out = np.empty((6, 6))
    assert lib.gpx_gp_dlh_d2lh(g._dev.handle, None, _lib.dptr(out), None) == _lib.ERR_UNSUPPORTED
    dm = np.empty((6, Xo.shape[0]))
    assert lib.gpx_gp_dm_dtheta(g._dev.handle, _lib.dptr(np.ascontiguousarray(Xo)), Xo.shape[0], _lib.dptr(dm)) == _lib.ERR_UNSUPPORTED
    h = ctypes.c_void_p()
    assert lib.gpx_gp_create(ctypes.byref(h), _lib.F64, _lib.KERNEL_GAUSSIAN_ARD, 100, 65) == _lib.ERR_ARG
    assert not h
    assert lib.gpx_gp_create(ctypes.byref(h), _lib.F64, _lib.KERNEL_GAUSSIAN_ARD, 100, 64) == _lib.OK
    lib.gpx_gp_destroy(h)
    mg = ctypes.c_void_p()
    assert lib.gpx_mg_create_local(ctypes.byref(mg), _lib.F64, _lib.KERNEL_GAUSSIAN_ARD, 1024, 4, 256, 1, 0) == _lib.ERR_ARG
    K = np.empty((Xo.shape[0], X.shape[0]))
    p = np.ascontiguousarray(k.params)
    for member in (_lib.DK_DH, _lib.DK_DW, _lib.D2K_DWDW):
        assert lib.gpx_kmat_host(_lib.KERNEL_GAUSSIAN_ARD, member, _lib.dptr(K), _lib.dptr(np.ascontiguousarray(Xo)), Xo.shape[0],
                                 _lib.dptr(np.ascontiguousarray(X)), X.shape[0], 4, _lib.dptr(p), 0.0) == _lib.ERR_UNSUPPORTED


def test_d_kmat_on_device_pointers():
    """gpx_d_kmat accepts the family for GPX_K (scaling into the thread's scratch) and refuses the other members."""
    lib = _lib.load()
    n, m, d = 130, 70, 5
    X, _, Xo = _data(n, d, m)
    k = gp.GaussianARDKernel(1.3, _widths(d))
    p = np.ascontiguousarray(k.params)
    ld = 80
    bufs = [ctypes.c_void_p() for _ in range(3)]
    for b, nbytes in zip(bufs, (X.nbytes, Xo.nbytes, n * ld * 8)):
        _lib.check(lib.gpx_malloc(ctypes.byref(b), nbytes))
    try:
        _lib.check(lib.gpx_memcpy_h2d(bufs[0], X.ctypes.data_as(ctypes.c_void_p), X.nbytes, None))
        _lib.check(lib.gpx_memcpy_h2d(bufs[1], Xo.ctypes.data_as(ctypes.c_void_p), Xo.nbytes, None))
        _lib.check(lib.gpx_d_kmat(_lib.F64, _lib.KERNEL_GAUSSIAN_ARD, _lib.K, bufs[0], n, bufs[1], m, d, _lib.dptr(p), 0.0, _lib.FULL,
                                  bufs[2], ld, None))
        out = np.empty((n, ld))
        _lib.check(lib.gpx_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), bufs[2], out.nbytes, None))
        _lib.check(lib.gpx_device_sync())
        assert lib.gpx_d_kmat(_lib.F64, _lib.KERNEL_GAUSSIAN_ARD, _lib.DK_DW, bufs[0], n, bufs[1], m, d, _lib.dptr(p), 0.0, _lib.FULL,
                              bufs[2], ld, None) == _lib.ERR_UNSUPPORTED
    finally:
        for b in bufs:
            lib.gpx_free(b)
    np.testing.assert_array_equal(out[:, :m], k(X, Xo))
    np.testing.assert_allclose(out[:, :m], ard_K(X, Xo, 1.3, k.w), rtol=1e-12, atol=1e-300)
