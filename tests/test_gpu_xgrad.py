"""GPU tests of the input-space gradients: the backward sweep X <- X L^-1 alone (gpx_d_trsm_right_l), and GP.dmean_dx /
GP.dvar_dx / GP.predict_grad (gpx_gp_mean_grad, gpx_gp_var_grad, gpx_d_pred_grad) against the numpy closed forms of
tests/_xgrad_helpers.py, which tests/test_xgrad_cpu.py anchors against central differences of the oracle.

Tolerances: the sweep's componentwise residual bound is the textbook gamma_n bound with room for the block products,
16 n eps (|X_out| |L|); fp64 gradients against the closed forms carry the project's own rtol 1e-7 / atol 1e-10 (ORACLE_TOL of
tests/test_gpu_var.py); two device evaluations of the same quantity agree within 1e-10 max|ref| (tests/test_gpu_dist_cov.py)."""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from gaussian_processes_amd.device import DeviceBuffer, sync
from oracle import gp_oracle as orc
from conftest import load_golden
from _xgrad_helpers import RefGP, central_differences

pytestmark = pytest.mark.gpu

ORACLE_TOL = dict(rtol=1e-7, atol=1e-10)
NPDT = {"float64": np.float64, "float32": np.float32}
DTID = {"float64": _lib.F64, "float32": _lib.F32}


def _round_up(v, m):
    return (v + m - 1) // m * m


# ---- 1. the sweep alone ----
def _sweep(entry, dtype, L, X, ldl, ldx):
    """entry(L, X) through the device, in place on a padded copy of X; the padding must come back untouched."""
    n, m = L.shape[0], X.shape[0]
    Lp, Xp = np.zeros((n, ldl), dtype=L.dtype), np.full((m, ldx), 7.0, dtype=X.dtype)
    Lp[:, :n], Xp[:, :n] = L, X
    dL, dX = DeviceBuffer.from_host(Lp), DeviceBuffer.from_host(Xp)
    _lib.check(getattr(_lib.load(), entry)(DTID[str(L.dtype)], dL.ptr, n, ldl, dX.ptr, m, ldx, None))
    sync()
    out = dX.to_host()
    assert (out[:, n:] == 7.0).all()
    return out[:, :n].astype(np.float64)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 777, 1100])
def test_sweep_componentwise_residual(n, dtype):
    rng = np.random.RandomState(n)
    npdt, eps = NPDT[dtype], float(np.finfo(NPDT[dtype]).eps)
    L = (np.tril(rng.randn(n, n)) / np.sqrt(n) + 2.0 * np.eye(n)).astype(npdt)      # every diagonal block well conditioned
    L64, ldl, ldx = L.astype(np.float64), _round_up(n, 16), _round_up(n, 16) + 16
    for m in (1, 7, 130):
        X = rng.randn(m, n).astype(npdt)
        X64 = X.astype(np.float64)
        for entry, Lop in (("gpx_d_trsm_right_l", L64), ("gpx_d_trsm_right_lt", L64.T)):
            out = _sweep(entry, dtype, L, X, ldl, ldx)
            res, bound = np.abs(out @ Lop - X64), 16.0 * n * eps * (np.abs(out) @ np.abs(Lop))
            worst = float((res / bound).max())
            print("%s n=%d m=%d %s: max residual / bound = %.3e" % (entry, n, m, dtype, worst))
            assert np.isfinite(out).all()
            assert (res <= bound).all(), (entry, n, m, worst)


def test_sweep_is_repeatable():
    rng = np.random.RandomState(5)
    n, m = 777, 130
    L = np.tril(rng.randn(n, n)) / np.sqrt(n) + 2.0 * np.eye(n)
    X = rng.randn(m, n)
    a = _sweep("gpx_d_trsm_right_l", "float64", L, X, 784, 800)
    b = _sweep("gpx_d_trsm_right_l", "float64", L, X, 784, 800)
    assert np.array_equal(a, b)


# ---- 2. gradients against the closed forms ----
FAMILIES = {
    "gaussian-d1": ("gaussian", 1, (1.0, 0.5)),
    "gaussian-d3": ("gaussian", 3, (1.0, 0.5 * np.sqrt(3))),
    "periodic-d1": ("periodic", 1, (1.0, 0.8, 3.0)),
    "periodic-d2": ("periodic", 2, (1.0, 0.8, 3.0)),
    "ard-d3": ("ard", 3, (1.2, 0.6, 1.15, 1.7)),
}
MS = [0, 1, 77, 300]
_CASES = {}


def _kernel(kind, params):
    if kind == "gaussian":
        return gp.GaussianKernel(*params)
    if kind == "periodic":
        return gp.PeriodicKernel(*params)
    return gp.GaussianARDKernel(params[0], np.array(params[1:]))


def _pts(P, d, kind):
    return P.ravel() if (d == 1 and kind != "ard") else P


def _case(kind, d, params, N, m=max(MS), s=1.0):
    """(X, y, Xo, the reference's (dmean_dx, dvar_dx) at all test points, the reference), one CPU evaluation per case."""
    key = (kind, d, params, N, m)
    if key not in _CASES:
        X, y, Xo = orc.synth_inputs(N, d, m)
        ref = RefGP(kind, params, X, y, s)
        _CASES[key] = (X, y, Xo, ref.grads(Xo), ref)
    return _CASES[key]


def _gp(kind, d, params, X, y, dtype="float64", s=1.0):
    return gp.GP(_kernel(kind, params), _pts(X, d, kind), y, s=s, dtype=dtype)


@pytest.mark.parametrize("N", [1000, 1024, 1536])
@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_gradients_against_the_closed_forms(fam, N):
    kind, d, params = FAMILIES[fam]
    X, y, Xo, (gm, gv), _ = _case(kind, d, params, N)
    g = _gp(kind, d, params, X, y)
    g.log_lh                                                  # fit
    for m in MS:
        xo = _pts(Xo[:m], d, kind)
        shape = xo.shape
        got_m = g.dmean_dx(xo)
        assert got_m.shape == shape and got_m.dtype == np.float64
        np.testing.assert_allclose(got_m.reshape(m, d), gm[:m], **ORACLE_TOL)
        for chunk_rows in (0, 128):
            _lib.route_reset()
            got_v = g.dvar_dx(xo, chunk_rows=chunk_rows)
            assert got_v.shape == shape and got_v.dtype == np.float64
            np.testing.assert_allclose(got_v.reshape(m, d), gv[:m], **ORACLE_TOL)
            chunks = 0 if m == 0 else (1 if (chunk_rows == 0 or m <= 128) else -(-m // 128))
            assert _lib.route_count(_lib.ROUTE_GRAD_CHUNK) == chunks
            assert _lib.route_count(_lib.ROUTE_VAR_CHUNK) == 0
            # the operator route of the new sweep from two operator blocks on, one hit per sweep, and only there
            assert _lib.route_count(_lib.ROUTE_TRSM_L_OPS) == (chunks if N in (1024, 1536) else 0)
            assert _lib.route_count(_lib.ROUTE_TRSM_OPS) == (chunks if N in (1024, 1536) else 0)


# one Gaussian case per bracket of the fused kernel (d <= 4: four points a workgroup; d <= 16: one window; beyond: windows
# of 16, d = 17 the first ragged one, d = 32 the flagship) and the largest d the mean kernel's LDS chunk admits per dtype.
# w = 3 sqrt(d), h = 3: the kernel is wide enough that every training point contributes (gradients ~ 1e-2, not 1e-60).
BRACKET_D = [4, 5, 16, 17, 32, 47]


@pytest.mark.parametrize("d", BRACKET_D)
def test_gradient_brackets_of_d(d):
    params = (3.0, 3.0 * np.sqrt(d))
    X, y, Xo, (gm, gv), _ = _case("gaussian", d, params, 1000, 77)
    assert np.abs(gm).max() > 1e-4 and np.abs(gv).max() > 1e-6
    g = _gp("gaussian", d, params, X, y)
    np.testing.assert_allclose(g.dmean_dx(Xo), gm, **ORACLE_TOL)
    np.testing.assert_allclose(g.dvar_dx(Xo), gv, **ORACLE_TOL)


def _pred_grad_direct(dtype, d, m=5, n=300):
    """gpx_d_pred_grad itself on gaussian points with weights alpha: (status, device result, numpy closed form)."""
    from _xgrad_helpers import dK_dxo
    npdt = NPDT[dtype]
    X, y, Xo = orc.synth_inputs(n, d, m)
    X, Xo, alpha = X.astype(npdt), Xo.astype(npdt), np.random.RandomState(d).randn(n).astype(npdt)
    params = np.array([3.0, 3.0 * np.sqrt(d)])
    dxo, dx, da, out = DeviceBuffer.from_host(Xo), DeviceBuffer.from_host(X), DeviceBuffer.from_host(alpha), DeviceBuffer((m, d)).zero()
    rc = _lib.load().gpx_d_pred_grad(DTID[dtype], _lib.KERNEL_GAUSSIAN, dxo.ptr, m, dx.ptr, n, d, _lib.dptr(params), da.ptr, None, 0,
                                     1.0, out.ptr, None)
    sync()
    X64, Xo64 = X.astype(np.float64), Xo.astype(np.float64)
    K = orc.kernel_matrix("gaussian", "K", Xo64, X64, tuple(params))
    return rc, out.to_host(), np.einsum("ijk,j->ik", dK_dxo("gaussian", tuple(params), Xo64, X64, K), alpha.astype(np.float64))


def test_range_of_d_is_the_mean_kernels():
    """Every d gpx_d_mean takes for the dtype (its LDS chunk: d * 257 * es <= 96 KiB -- 47 in fp64, 95 in fp32), and a refusal
    beyond.  (A float32 FIT stops at d = 94, the kernel build's own tile: 95 is reached through the device entry.)"""
    rc, got, ref = _pred_grad_direct("float64", 47)
    assert rc == _lib.OK
    np.testing.assert_allclose(got, ref, **ORACLE_TOL)
    rc, got, ref = _pred_grad_direct("float32", 95)
    assert rc == _lib.OK and np.abs(ref).max() > 1e-3
    np.testing.assert_allclose(got, ref, rtol=1e-2, atol=5e-3 * max(1.0, float(np.abs(ref).max())))
    for dtype, d in (("float64", 48), ("float32", 96)):
        assert _pred_grad_direct(dtype, d)[0] == _lib.ERR_UNSUPPORTED
        assert "too large" in _lib.last_error()
    X, y, Xo = orc.synth_inputs(300, 48, 5)
    g = gp.GP(gp.GaussianKernel(3.0, 3.0 * np.sqrt(48)), X, y, s=1.0)
    for f in (g.mean, g.dmean_dx, g.dvar_dx):
        with pytest.raises(NotImplementedError, match="too large"):
            f(Xo)


# ---- 3. fp32 ----
# |fp32 - fp64 device result| <= F32_C * max(1, max|fp64 result|).  The bound is not derivable (it is the conditioning of the
# two sweeps in fp32): F32_C is 4 x the largest figure measured over these cases on an MI355X, for box-to-box route differences.
#   measured, largest over the cases: dmean_dx 6.94e-7 / 1.079 = 6.4e-7 (gaussian-d1, N = 1024),
#                                     dvar_dx  8.91e-7 (gaussian-d1, N = 1000)            F32_C = 4 x 8.91e-7
# The project's fp32 tolerance for `var` (rtol 1e-2, atol 5e-3 max(1, max|ref|)) is asserted against the closed forms as well;
# the measured figures are four orders of magnitude inside it.
F32_C = 3.6e-6
F32_CASES = [(fam, N) for fam in sorted(FAMILIES) for N in (1000, 1024)] + [("gaussian-d3", 1536)]


@pytest.mark.parametrize("fam,N", F32_CASES, ids=["%s-%d" % c for c in F32_CASES])
def test_fp32_against_fp64_on_the_device(fam, N):
    kind, d, params = FAMILIES[fam]
    X, y, Xo, (gm, gv), _ = _case(kind, d, params, N)
    g64, g32 = _gp(kind, d, params, X, y), _gp(kind, d, params, X, y, dtype="float32")
    xo = _pts(Xo, d, kind)
    for name, f64, f32, ref in (("dmean_dx", g64.dmean_dx(xo), g32.dmean_dx(xo), gm), ("dvar_dx", g64.dvar_dx(xo), g32.dvar_dx(xo), gv)):
        f64, f32 = f64.reshape(-1, d), f32.reshape(-1, d)
        err, scale = float(np.abs(f32 - f64).max()), max(1.0, float(np.abs(f64).max()))
        print("fp32 %s %s N=%d: |fp32 - fp64| = %.3e, scale %.3e" % (name, fam, N, err, scale))
        assert f32.dtype == np.float64
        np.testing.assert_allclose(f32, ref, rtol=1e-2, atol=5e-3 * max(1.0, float(np.abs(ref).max())))
        assert err <= F32_C * scale, (name, err, F32_C * scale)


def test_fp32_at_the_largest_d_a_float32_fit_takes():
    d = 94
    params = (3.0, 3.0 * np.sqrt(d))
    X, y, Xo, (gm, gv), _ = _case("gaussian", d, params, 1000, 77)
    g = _gp("gaussian", d, params, X, y, dtype="float32")
    for name, got, ref in (("dmean_dx", g.dmean_dx(Xo), gm), ("dvar_dx", g.dvar_dx(Xo), gv)):
        print("fp32 %s d=%d: |fp32 - closed form| = %.3e, max|ref| %.3e" % (name, d, np.abs(got - ref).max(), np.abs(ref).max()))
        np.testing.assert_allclose(got, ref, rtol=1e-2, atol=5e-3 * max(1.0, float(np.abs(ref).max())))


# ---- 4. an independent cross-check on the device ----
@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_against_central_differences_of_the_devices_own_mean_and_var(fam):
    kind, d, params = FAMILIES[fam]
    X, y, Xo, _, _ = _case(kind, d, params, 1000)
    g = _gp(kind, d, params, X, y)
    P = Xo[:5]
    for name, got, f in (("mean", g.dmean_dx(_pts(P, d, kind)), g.mean), ("var", g.dvar_dx(_pts(P, d, kind)), g.var)):
        fd = central_differences(lambda p: f(_pts(p, d, kind)), P, 1e-5)
        got = got.reshape(5, d)
        err, bound = float(np.abs(got - fd).max()), 1e-7 * max(1.0, float(np.abs(got).max()))
        print("device d%s/dx %s: |analytic - fd| %.3e, bound %.3e" % (name, fam, err, bound))
        assert err <= bound, (name, err, bound)


# ---- 5. exactness and consistency ----
def test_a_point_beyond_every_clamp_has_gradients_exactly_zero():
    kind, d, params = FAMILIES["gaussian-d3"]
    for N in (1000, 1024):
        X, y, Xo, _, _ = _case(kind, d, params, N)
        g = _gp(kind, d, params, X, y)
        far = np.vstack([Xo[:2], X.max(0)[None] + 100.0])       # exp(-r^2 / 2 w^2) with r > 170, w < 1: clamped to exactly 0
        gm, gv = g.dmean_dx(far), g.dvar_dx(far)
        assert (gm[2] == 0.0).all() and (gv[2] == 0.0).all()
        assert (gm[:2] != 0.0).all() and (gv[:2] != 0.0).all()


def test_repeatability_chunking_predict_grad_noise_and_checkpoint(tmp_path):
    kind, d, params = FAMILIES["gaussian-d3"]
    X, y, Xo, (gm, gv), ref = _case(kind, d, params, 1024)
    g = _gp(kind, d, params, X, y, s=1.0)
    m1, v1 = g.dmean_dx(Xo), g.dvar_dx(Xo)
    assert np.array_equal(m1, g.dmean_dx(Xo)) and np.array_equal(v1, g.dvar_dx(Xo))            # two calls: bitwise
    assert np.abs(g.dvar_dx(Xo, chunk_rows=128) - v1).max() <= 1e-10 * np.abs(gv).max()       # three chunks against one
    mean, var, dm, dv = g.predict_grad(Xo)
    tol = 1e-10
    assert np.abs(mean - g.mean(Xo)).max() <= tol * max(1.0, np.abs(mean).max())
    assert np.abs(var - g.var(Xo)).max() <= tol * max(1.0, np.abs(var).max())
    assert np.abs(dm - m1).max() <= tol * np.abs(gm).max() and np.abs(dv - v1).max() <= tol * np.abs(gv).max()
    _, var_n, _, dv_n = g.predict_grad(Xo, noise=True, chunk_rows=128)
    np.testing.assert_allclose(var_n, var + 1.0, rtol=0, atol=1e-10)
    assert np.abs(dv_n - v1).max() <= tol * np.abs(gv).max()
    path = str(tmp_path / "fit.gpx")
    g.save_fitted(path)
    h = gp.GP.load_fitted(path)
    assert np.array_equal(h.dmean_dx(Xo), m1) and np.array_equal(h.dvar_dx(Xo), v1)
    hm, hv, hdm, hdv = h.predict_grad(Xo)
    assert np.array_equal(hv, var) and np.array_equal(hdv, dv)


def test_restored_ard_and_one_dimensional_shapes(tmp_path):
    kind, d, params = FAMILIES["ard-d3"]
    X, y, Xo, (gm, gv), _ = _case(kind, d, params, 1000)
    g = _gp(kind, d, params, X, y)
    path = str(tmp_path / "ard.gpx")
    g.save_fitted(path)
    h = gp.GP.load_fitted(path)
    np.testing.assert_allclose(h.dmean_dx(Xo[:77]), gm[:77], **ORACLE_TOL)
    np.testing.assert_allclose(h.dvar_dx(Xo[:77]), gv[:77], **ORACLE_TOL)
    kind, d, params = FAMILIES["periodic-d1"]
    X, y, Xo, (gm, gv), _ = _case(kind, d, params, 1000)
    g = _gp(kind, d, params, X, y)
    assert g.dmean_dx(Xo[:7].ravel()).shape == (7,) and g.dvar_dx(Xo[:7].ravel()).shape == (7,)
    assert g.dmean_dx(Xo[:7]).shape == (7, 1)
    assert all(a.shape == (0,) for a in g.predict_grad(np.zeros(0)))


def test_a_fit_that_is_not_positive_definite():
    rec = load_golden("gp_nonpd.npz")
    h, w, s = rec["params"]
    g = gp.GP(gp.GaussianKernel(h, w), rec["x"], rec["y"], s=s)
    xo = np.linspace(rec["x"].min(), rec["x"].max(), 5)
    for f in (g.dmean_dx, g.dvar_dx, g.predict_grad):
        with pytest.raises(np.linalg.LinAlgError):
            f(xo)
