"""GPU tests of the gradient of the leave-one-out criterion: GP.dloo_dtheta (gpx_gp_loo_grad, gpx_gp_loo_grad_weights), the
lock-step batch (gpx_gp_fit_batch_loo, mlii.BatchEvaluator.value_and_grad(criterion="loo")) and mlii.optimize(criterion="loo").

The yardstick is tests/_loograd_helpers.py (numpy, from the explicit inverse; its two forms and central differences agree in
tests/test_loograd_cpu.py).  Tolerances are the project's own: the golden records' C_COND * cond(Kxx) * eps * scale bound
with scale_j the sum of the absolute values of the terms that enter component j, rtol 1e-7 / atol 1e-10 (ORACLE_TOL) for fp64
against a closed form, the same C_COND bound with eps of float32 for fp32, rtol 1e-10 for batch against single handle
(tests/test_gpu_round6.py), and the central-difference line of tests/test_gpu_ard.py.  Wherever the C_COND bound is used
the test also asserts bound <= max_j |ref_j|: a bound that exceeds the gradient itself could hide a wrong sign.

Parameters.  That last assertion decides them: cond(K) ~ 1 + (a few eigenvalues ~ N h^2) / s^2 for a kernel matrix of low
numerical rank, and with 16 cond eps_f32 ~ 1e-3 cond the fp32 bound is vacuous beyond cond ~ 1e3.  The Gaussian kernel on
orc.synth_inputs (d = 3, w = 0.5 sqrt(d): near-diagonal) stays below 2e2 at h = 1 for both s.  The periodic kernel in one
dimension has a handful of significant eigenvalues whatever N: h = s / 2 keeps cond at 1.3e2 for N = 1350 (h = 1, s = 0.1
gives 5e4 and a bound of 1e4 |ref|).  ARD: h = 0.4, widths in [0.3, 3] on the inputs / 10 for d >= 32 (tests/test_gpu_ard.py)
and on the inputs / 3 for d = 3, 12, where / 10 makes K numerically low-rank.  With these the fp32 bound is at most 3.5 % of
max |ref| in every case (evaluated in numpy)."""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib, mlii
from oracle import gp_oracle as orc
from conftest import load_golden
from test_dist_gp_cpu import _PythonRBF
from test_gpu_var import C_COND, GOLDEN_CASES, ORACLE_TOL, _records
from _ard_helpers import ard_K, ard_dK
from _loograd_helpers import loo_grad_from_inverse, loo_grad_reference, with_noise

pytestmark = pytest.mark.gpu

_EPS = {"float64": float(np.finfo(np.float64).eps), "float32": float(np.finfo(np.float32).eps)}


def _c_loo_grad(g):
    """(value, gradient) straight from gpx_gp_loo_grad on g's fitted handle."""
    out, total = np.empty(len(g.params)), ctypes.c_double(0.0)
    _lib.check(_lib.load().gpx_gp_loo_grad(g._fit().handle, ctypes.byref(total), _lib.dptr(out)))
    return np.float64(total.value), out


def _c_weights(g):
    G = np.empty((g._n, g._n))
    _lib.check(_lib.load().gpx_gp_loo_grad_weights(g._fit().handle, _lib.dptr(G), g._n))
    return G


def _check_bound(got, ref, scale, cond, dtype, what):
    bound = C_COND * cond * _EPS[dtype] * scale
    err = np.abs(np.asarray(got) - ref)
    print("%s %s: cond %.2e\n  got %s\n  ref %s\n  err %s\n  bound %s\n  largest err / bound %.3f, largest bound / max|ref| %.2e"
          % (what, dtype, cond, got, ref, err, bound, (err / bound).max(), bound.max() / np.abs(ref).max()))
    assert bound.max() <= np.abs(ref).max(), "%s: the bound exceeds the gradient itself" % what
    assert (err <= bound).all(), "%s: |got - ref| exceeds C_COND cond eps scale" % what


# ---- 1. the golden records ----
@pytest.mark.parametrize("prefix,make_kernel", GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_dloo_golden_gp_small(prefix, make_kernel):
    rec = _records(load_golden("gp_small.npz"), prefix)
    kp, s = rec["params"][:-1], rec["params"][-1]
    kind = "periodic" if make_kernel is gp.PeriodicKernel else "gaussian"
    J = orc.jacobian(kind, rec["x"], rec["x"], np.asarray(kp, dtype=np.float64))
    value, ref, _, scale = loo_grad_from_inverse(rec["inv_Kxx"], rec["inv_Kxx_y"], with_noise(J, s))
    g = gp.GP(make_kernel(*kp), rec["x"], rec["y"], s=s)
    got = g.dloo_dtheta
    assert got.shape == ref.shape and got.dtype == np.float64
    _check_bound(got, ref, scale, float(np.linalg.cond(rec["Kxx"])), "float64", prefix)
    np.testing.assert_allclose(g.loo_log_lh, value, rtol=1e-10)


# ---- 2. the closed form on synthetic inputs ----
_CASES = {}


def _widths(d):
    return np.random.RandomState(7).uniform(0.3, 3.0, d)


def _case(kind, N, d, s):
    """x, y, a kernel factory and the numpy reference (value, gradient, G, scale, cond): one CPU evaluation per case."""
    key = (kind, N, d, s)
    if key not in _CASES:
        X, y, _ = orc.synth_inputs(N, d, 1)
        if kind == "ard":
            X = X / (10.0 if d >= 32 else 3.0)
            h, w = 0.4, _widths(d)
            K = ard_K(X, X, h, w) + s * s * np.eye(N)
            dKs = with_noise(ard_dK(X, h, w), s)
            make = lambda: gp.GaussianARDKernel(h, w)       # noqa: E731
        else:
            kp = np.array([1.0, 0.5 * np.sqrt(d)]) if kind == "gaussian" else np.array([0.5 * s, 0.8, 3.0])
            K = orc.OracleGP(kind, tuple(kp), X, y, s).Kxx
            dKs = with_noise(orc.jacobian(kind, X, X, kp), s)
            cls = gp.GaussianKernel if kind == "gaussian" else gp.PeriodicKernel
            make = lambda: cls(*kp)                         # noqa: E731
        ref = loo_grad_reference(K, dKs, y) + (float(np.linalg.cond(K)),)
        _CASES[key] = (X.ravel() if d == 1 else X, y, make, ref)
    return _CASES[key]


SHAPES = [("gaussian", N, 3) for N in (40, 130, 700, 1350)] + [("periodic", N, 1) for N in (40, 130, 700, 1350)] + \
         [("ard", 700, 3), ("ard", 700, 12), ("ard", 1000, 32), ("ard", 1000, 40)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("s", [1.0, 0.1])
@pytest.mark.parametrize("kind,N,d", SHAPES, ids=["%s-%d-%d" % c for c in SHAPES])
def test_dloo_against_the_closed_form(kind, N, d, s, dtype):
    x, y, make, (value, ref, _, scale, cond) = _case(kind, N, d, s)
    g = gp.GP(make(), x, y, s=s, dtype=dtype)
    got = g.dloo_dtheta
    assert got.shape == ref.shape and got.dtype == np.float64
    what = "%s N=%d d=%d s=%g" % (kind, N, d, s)
    if dtype == "float64":
        print("%s: cond %.2e\n  got %s\n  ref %s\n  rel %s" % (what, cond, got, ref, np.abs(got - ref) / np.abs(ref)))
        np.testing.assert_allclose(got, ref, **ORACLE_TOL["float64"])
    else:
        _check_bound(got, ref, scale, cond, dtype, what)
    # the value came with it, and it is the leave-one-out call's own, bit for bit, whichever of the two ran first
    assert "loo_log_lh" in g._memoized
    np.testing.assert_allclose(g.loo_log_lh, value, **ORACLE_TOL[dtype])
    from_grad = np.float64(g.loo_log_lh)
    g.loo()                                                 # refills the member from gpx_gp_loo
    assert np.float64(g._memoized["loo_log_lh"]).tobytes() == from_grad.tobytes()
    g2 = gp.GP(make(), x, y, s=s, dtype=dtype)
    v2, first = _c_loo_grad(g2)                             # gradient first, on a handle that has no diagonal yet
    assert np.float64(g2.loo_log_lh).tobytes() == v2.tobytes() == np.float64(g.loo_log_lh).tobytes()
    g3 = gp.GP(make(), x, y, s=s, dtype=dtype)
    v3 = np.float64(g3.loo_log_lh)                          # leave-one-out first
    assert _c_loo_grad(g3)[0].tobytes() == v3.tobytes()
    # two calls, and a second GP on the same data: the same bytes
    assert first.tobytes() == got.tobytes() and _c_loo_grad(g2)[1].tobytes() == got.tobytes()
    del g.dloo_dtheta
    assert g.dloo_dtheta.tobytes() == got.tobytes()


# ---- 3. the weights themselves ----
class _PythonRBFJ(_PythonRBF):
    """_PythonRBF with its Jacobian: k = h^2 exp(-r^2 / (2 l^2)), dk/dh = 2 k / h, dk/dl = k r^2 / l^3."""

    def jacobian(self, x1, x2, out=None):
        a = np.asarray(x1, dtype=np.float64).reshape(len(x1), -1)
        b = np.asarray(x2, dtype=np.float64).reshape(len(x2), -1)
        r2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        k = self.K(x1, x2)
        return np.array([2.0 * k / self.h, k * r2 / self.ell ** 3])


@pytest.mark.parametrize("N", [130, 700])
def test_loo_grad_weights_against_numpy(N):
    x, y, make, (_, ref, Gref, _, cond) = _case("gaussian", N, 3, 1.0)
    g = gp.GP(make(), x, y, s=1.0)
    G = _c_weights(g)
    err, bound = float(np.abs(G - Gref).max()), C_COND * cond * _EPS["float64"] * float(np.abs(Gref).max())
    print("G at N = %d: err %.3e bound %.3e" % (N, err, bound))
    assert err <= bound
    assert G.tobytes() == np.ascontiguousarray(G.T).tobytes()
    assert _c_weights(g).tobytes() == G.tobytes()
    # the contraction on the host is the device's gradient (the host route of GP.dloo_dtheta, spelt out)
    J = orc.jacobian("gaussian", x, x, g.K.params)
    host = np.array([np.sum(J[0] * G), np.sum(J[1] * G), 2.0 * np.trace(G)])
    np.testing.assert_allclose(host, g.dloo_dtheta, rtol=1e-10)


def test_loo_grad_weights_need_only_a_factor(tmp_path):
    N, d, s = 130, 3, 1.0
    X, y, _ = orc.synth_inputs(N + 6, d, 1)
    tol = C_COND * _EPS["float64"]

    def check(g, what):
        K = np.asarray(g.Kxx)
        Gref = loo_grad_reference(K, [], g.y)[2]
        G = _c_weights(g)
        err, bound = float(np.abs(G - Gref).max()), tol * float(np.linalg.cond(K)) * float(np.abs(Gref).max())
        print("%s: n = %d, err %.3e bound %.3e" % (what, len(g.y), err, bound))
        assert G.shape == Gref.shape and err <= bound and G.tobytes() == np.ascontiguousarray(G.T).tobytes()

    w = 0.5 * np.sqrt(d)
    base = gp.GP(gp.GaussianKernel(1.0, w), X[:N], y[:N], s=s)
    check(base, "a fit")
    path = str(tmp_path / "fit.gpx")
    base.save_fitted(path)
    check(gp.GP.load_fitted(path), "a restored checkpoint")
    check(base.extend(X[N:], y[N:]), "extend")
    check(base.remove([3, 64, 129]), "remove")
    # a kernel the library knows nothing about: fitted from the uploaded matrix, differentiated on the host
    hp = np.sqrt(1.0 / (w * np.sqrt(2.0 * np.pi)))          # the plugin's h for the native kernel's (h = 1, w)
    plug = gp.GP(_PythonRBFJ(hp, w), X[:N], y[:N], s=s)
    check(plug, "a plugin kernel (gpx_gp_set_K)")
    nat = base.dloo_dtheta
    # chain rule between the two parametrisations: h_native = h_plugin sqrt(w sqrt(2 pi)), at fixed h_plugin dh_native/dw = h_native / (2 w)
    expect = np.array([nat[0] * np.sqrt(w * np.sqrt(2.0 * np.pi)), nat[1] + nat[0] * 1.0 / (2.0 * w), nat[2]])
    got = plug.dloo_dtheta
    print("plugin %s\nnative, in the plugin's parameters %s" % (got, expect))
    np.testing.assert_allclose(got, expect, rtol=1e-10)
    np.testing.assert_allclose(plug.loo_log_lh, base.loo_log_lh, rtol=1e-10)
    lib, out = _lib.load(), np.empty(3)
    assert lib.gpx_gp_loo_grad(plug._fit().handle, _lib.dptr(out), _lib.dptr(out)) == _lib.ERR_ARG      # no kernel in that handle


# ---- 4. central differences of the device's own criterion ----
def test_dloo_central_differences_of_the_device_loo_log_lh():
    N, d = 700, 5
    X, y, _ = orc.synth_inputs(N, d, 48)
    X = X / 10.0
    theta = np.concatenate([[1.3], _widths(d), [0.7]])
    g = gp.GP(gp.GaussianARDKernel(theta[0], theta[1:-1]), X, y, s=theta[-1])
    grad = np.array(g.dloo_dtheta)
    fd = np.empty(d + 2)
    for i in range(d + 2):
        v = []
        for sgn in (-1.0, 1.0):
            t = theta.copy(); t[i] *= 1.0 + sgn * 1e-5
            g.params = t
            v.append(float(g.loo_log_lh))
        fd[i] = (v[1] - v[0]) / (2e-5 * theta[i])
    print("dloo_dtheta %s\ncentral differences %s" % (grad, fd))
    np.testing.assert_allclose(grad, fd, rtol=2e-5, atol=1e-6 * np.abs(grad).max())


# ---- 5. the lock-step batch ----
def _batch_case(kernel, N, d):
    X, y, _ = orc.synth_inputs(N, d, 1)
    if kernel == "gaussian":
        th = np.array([[1.0, 0.9, 1.0], [1.0, 0.0, 1.0], [1.3, 1.2, 0.5], [1.0, 1e4, 0.0], [0.7, 0.6, 0.3]])
        return X, y, th, lambda r: gp.GaussianKernel(r[0], r[1])
    X = X / 10.0
    w = _widths(d)
    th = np.array([np.concatenate([[1.3], w, [0.7]]), np.concatenate([[1.0, 0.0], w[1:], [1.0]]),
                   np.concatenate([[1.0], np.full(d, 1e4), [0.0]])])
    return X, y, th, lambda r: gp.GaussianARDKernel(r[0], r[1:-1])


# (N = 1024: whole 512-column operator blocks, where a group's K^-1 and Y Y^T products run in lock-step; N = 700: row by row)
@pytest.mark.parametrize("kernel,N,d", [("gaussian", 700, 3), ("gaussian_ard", 700, 5), ("gaussian", 1024, 3)])
def test_fit_batch_loo_against_single_handles(kernel, N, d):
    X, y, th, make = _batch_case(kernel, N, d)
    bad, nonpd = 1, (3 if kernel == "gaussian" else 2)
    with mlii.BatchEvaluator(X, y, kernel=kernel) as ev:
        before_v, before_vg = ev(th), ev.value_and_grad(th)
        val, grad = ev.value_and_grad(th, criterion="loo")
        val2, grad2 = ev.value_and_grad(th, clamp=False, criterion="loo")
        assert val.tobytes() == val2.tobytes() == ev.loo(th).tobytes() and grad.tobytes() == grad2.tobytes()
        # the marginal-likelihood entries return what they returned before the leave-one-out call
        assert ev(th).tobytes() == before_v.tobytes()
        again = ev.value_and_grad(th)
        assert again[0].tobytes() == before_vg[0].tobytes() and again[1].tobytes() == before_vg[1].tobytes()
        info = np.zeros(len(th), dtype=np.int32)
        v3, g3 = np.empty(len(th)), np.empty_like(grad)
        _lib.check(ev.lib.gpx_gp_fit_batch_loo(ev.h, _lib.dptr(th), len(th), _lib.dptr(v3), _lib.dptr(g3),
                                               info.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        assert info[bad] == -1 and info[nonpd] > 0 and (np.delete(info, [bad, nonpd]) == 0).all()
    assert grad.shape == th.shape
    assert np.isnan(val[bad]) and np.isnan(grad[bad]).all()
    assert np.isneginf(val[nonpd]) and np.isnan(grad[nonpd]).all()
    for i in range(len(th)):
        if i in (bad, nonpd):
            continue
        g = gp.GP(make(th[i]), X, y, s=th[i, -1])
        print("row %d: batch %s %r\n       single %s %r" % (i, grad[i], val[i], g.dloo_dtheta, g.loo_log_lh))
        np.testing.assert_allclose(grad[i], g.dloo_dtheta, rtol=1e-10)
        np.testing.assert_allclose(val[i], g.loo_log_lh, rtol=1e-10)
        if N == 1024 and i == 0:
            # (the one size here whose products take the aligned route of the matrix-core kernel: against numpy too)
            K = orc.OracleGP("gaussian", tuple(th[i, :-1]), X, y, th[i, -1]).Kxx
            ref = loo_grad_reference(K, with_noise(orc.jacobian("gaussian", X, X, th[i, :-1].copy()), th[i, -1]), y)
            np.testing.assert_allclose(grad[i], ref[1], **ORACLE_TOL["float64"])
            np.testing.assert_allclose(val[i], ref[0], **ORACLE_TOL["float64"])


# ---- 6. the optimiser ----
def test_mlii_optimize_on_the_leave_one_out_criterion():
    N, d = 300, 2
    X, y, _ = orc.synth_inputs(N, d, 1)
    th0 = np.array([[1.0, 0.7, 1.0], [0.5, 1.5, 0.5], [2.0, 1.0, 0.3], [1.0, 2.5, 2.0]])
    res = mlii.optimize(X, y, th0, criterion="loo", maxiter=15)
    print(res)
    assert res["criterion"] == "loo" and res["theta"].shape == (4, 3)
    assert (res["log_lh"] >= res["log_lh0"]).all() and np.isfinite(res["log_lh"]).all()
    assert (res["log_lh"] > res["log_lh0"]).any()
    t = res["theta"][res["best"]]
    np.testing.assert_allclose(res["log_lh"][res["best"]], gp.GP(gp.GaussianKernel(t[0], t[1]), X, y, s=t[2]).loo_log_lh, rtol=1e-10)


# ---- 7. refusals ----
def test_dloo_refusals():
    rec = load_golden("gp_nonpd.npz")
    h, w, s = rec["params"]
    g = gp.GP(gp.GaussianKernel(h, w), rec["x"], rec["y"], s=s)
    got = g.dloo_dtheta
    assert got.shape == (3,) and np.isnan(got).all() and g.loo_log_lh == -np.inf
    v, c = _c_loo_grad(g)
    assert np.isneginf(v) and np.isnan(c).all()
    lib = _lib.load()
    out = np.empty(len(rec["y"]) ** 2)
    assert lib.gpx_gp_loo_grad_weights(g._fit().handle, _lib.dptr(out), len(rec["y"])) == _lib.ERR_ARG
    assert "not positive definite" in _lib.last_error()
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    with pytest.raises(NotImplementedError, match="use gp.GP"):
        gp.DistributedGP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1).dloo_dtheta
    # an unfitted handle; the periodic family beyond one dimension
    n = 24
    out = np.empty(n * n)
    X, y, _ = orc.synth_inputs(n, 2, 1)
    th = np.array([[1.0, 0.8, 3.0, 1.0]])
    for kernel, d, fitted, want in ((_lib.KERNEL_GAUSSIAN, 2, False, _lib.ERR_ARG), (_lib.KERNEL_PERIODIC, 2, True, _lib.ERR_UNSUPPORTED)):
        hd = ctypes.c_void_p()
        _lib.check(lib.gpx_gp_create(ctypes.byref(hd), _lib.F64, kernel, n, d))
        try:
            _lib.check(lib.gpx_gp_set_data(hd, _lib.dptr(np.ascontiguousarray(X)), _lib.dptr(y)))
            _lib.check(lib.gpx_gp_set_params(hd, _lib.dptr(th[0, :-1].copy()), 1.0))
            if fitted:
                _lib.check(lib.gpx_gp_fit(hd, None))
            assert lib.gpx_gp_loo_grad(hd, _lib.dptr(out), _lib.dptr(out[1:])) == want
            if fitted:
                assert lib.gpx_gp_fit_batch_loo(hd, _lib.dptr(th), 1, _lib.dptr(out), _lib.dptr(out[1:]), None) == want
                assert lib.gpx_gp_loo_grad_weights(hd, _lib.dptr(out), n) == _lib.OK      # the weights need no kernel
                K = np.empty((n, n))
                _lib.check(lib.gpx_gp_get_Kxx(hd, _lib.dptr(K), n))
                Gref = loo_grad_reference(K, [], y)[2]
                assert np.abs(out.reshape(n, n) - Gref).max() <= C_COND * np.linalg.cond(K) * _EPS["float64"] * np.abs(Gref).max()
            else:
                assert lib.gpx_gp_loo_grad_weights(hd, _lib.dptr(out), n) == want
        finally:
            lib.gpx_gp_destroy(hd)
