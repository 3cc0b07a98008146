"""GPU tests of leave-one-out cross-validation from the fitted factor: GP.inv_Kxx_diag / loo / loo_mean / loo_var /
loo_log_lh (gpx_gp_inv_diag, gpx_gp_loo, gpx_d_loo_rows).

Tolerances are the project's own: the golden records' C_COND * cond(Kxx) * eps * scale bound of tests/test_gpu_parity.py
with the scales of each derived quantity (first-order propagation of an error in K^-1 and alpha through
y - a / k, 1 / k and log(k) / 2 - a^2 / (2 k)), rtol 1e-7 / atol 1e-10 (fp32: 1e-2 / 5e-3) against a closed form, and
1e-10 * max between two device evaluations of the same quantity, the bound of tests/test_gpu_dist_cov.py."""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from oracle import gp_oracle as orc
from conftest import load_golden
from test_dist_gp_cpu import _PythonRBF
from test_gpu_var import C_COND, GOLDEN_CASES, ORACLE_TOL, _records
from _loo_helpers import loo_from_diag, loo_reference

pytestmark = pytest.mark.gpu

_EPS = np.finfo(np.float64).eps
_DTYPE_ID = {"float64": _lib.F64, "float32": _lib.F32}


def _check(names_got_ref, tol):
    for name, got, ref in names_got_ref:
        got, ref = np.asarray(got), np.asarray(ref)
        print("%s: max abs %.3e, max rel %.3e" % (name, np.abs(got - ref).max(), (np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)).max()))
        assert got.shape == ref.shape and got.dtype == np.float64
        np.testing.assert_allclose(got, ref, err_msg=name, **tol)


# ---- 1. the golden records ----
@pytest.mark.parametrize("prefix,make_kernel", GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_loo_golden_gp_small(prefix, make_kernel):
    rec = _records(load_golden("gp_small.npz"), prefix)
    kp, s = rec["params"][:-1], rec["params"][-1]
    Ki, alpha, y = rec["inv_Kxx"], rec["inv_Kxx_y"], rec["y"]
    kii = np.diag(Ki).copy()
    assert (kii > 0).all()
    mean, var, log_p = loo_from_diag(kii, alpha, y)
    tol = C_COND * float(np.linalg.cond(rec["Kxx"])) * _EPS
    amax, Kmax, kmin = np.abs(alpha).max(), np.abs(Ki).max(), kii.min()
    g = gp.GP(make_kernel(*kp), rec["x"], rec["y"], s=s)
    gm, gv, gl = g.loo()
    for name, got, ref, scale in (("inv_Kxx_diag", g.inv_Kxx_diag, kii, Kmax),
                                  ("loo_var", gv, var, Kmax / kmin ** 2),
                                  ("loo_mean", gm, mean, amax / kmin + amax * Kmax / kmin ** 2),
                                  ("log_p", gl, log_p, 0.5 * Kmax / kmin + amax ** 2 / kmin + 0.5 * amax ** 2 * Kmax / kmin ** 2)):
        err, bound = float(np.abs(got - ref).max()), tol * scale
        print("%s vs golden: err %.3e bound %.3e ratio %.3f" % (name, err, bound, err / bound))
        assert got.shape == ref.shape
        assert err <= bound, "%s: |got - ref| = %.3e exceeds C_COND cond eps scale = %.3e" % (name, err, bound)
    assert np.array_equal(g.loo_mean, gm) and np.array_equal(g.loo_var, gv)
    assert isinstance(g.loo_log_lh, np.float64)
    # the device's fixed-order sum of its own terms: any two summation orders of n terms differ by at most 2 n eps sum|x|
    assert abs(g.loo_log_lh - gl.sum()) <= 2 * len(y) * _EPS * np.abs(gl).sum()


# ---- 2. deleting every point in turn, on the device ----
@pytest.mark.parametrize("s", [1.0, 0.1])
@pytest.mark.parametrize("kind", ["gaussian", "periodic"])
def test_loo_equals_forty_refits_without_one_point(kind, s):
    n = 40
    d = 3 if kind == "gaussian" else 1
    X, y, _ = orc.synth_inputs(n, d, 1)
    x = X.ravel() if d == 1 else X
    make = (lambda: gp.GaussianKernel(1.0, 0.5 * np.sqrt(d))) if kind == "gaussian" else (lambda: gp.PeriodicKernel(1.0, 0.8, 3.0))
    g = gp.GP(make(), x, y, s=s)
    bmean, bvar = np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        m, v = gp.GP(make(), x[keep], y[keep], s=s).predict(x[i:i + 1], noise=True)
        bmean[i], bvar[i] = m[0], v[0]
    _check([("loo_mean", g.loo_mean, bmean), ("loo_var", g.loo_var, bvar)], ORACLE_TOL["float64"])


# ---- 3. the closed form: every route of the sweep, both dtypes ----
_CASES = {}


def _case(kind, N):
    """(x, y, make_kernel, the closed form from the oracle's Kxx), one CPU evaluation per (kind, N)."""
    if (kind, N) not in _CASES:
        d = 3 if kind == "gaussian" else 1
        X, y, _ = orc.synth_inputs(N, d, 1)
        kp = (1.0, 0.5 * np.sqrt(d)) if kind == "gaussian" else (1.0, 0.8, 3.0)
        make = gp.GaussianKernel if kind == "gaussian" else gp.PeriodicKernel
        ref = loo_reference(orc.OracleGP(kind, kp, X, y, 1.0).Kxx, y)
        _CASES[(kind, N)] = (X.ravel() if d == 1 else X, y, lambda: make(*kp), ref)
    return _CASES[(kind, N)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N", [1000, 1536, 4200])
@pytest.mark.parametrize("kind", ["gaussian", "periodic"])
def test_loo_against_the_closed_form(kind, N, dtype):
    x, y, make, (kii, mean, var, log_p) = _case(kind, N)
    lib = _lib.load()
    g = gp.GP(make(), x, y, s=1.0, dtype=dtype)
    h = g._fit_pd().handle
    _lib.route_reset()
    g.cov(x[:64])
    cov_ops = _lib.route_count(_lib.ROUTE_TRSM_OPS) > 0
    by_chunk = {}
    for chunk_rows in (0, 128, 512):
        # a new parameter set and back: the handle drops its diagonal, so every chunk size sweeps
        g.s = 2.0
        g.log_lh
        g.s = 1.0
        h = g._fit_pd().handle
        rows = _lib.var_plan(_DTYPE_ID[dtype], N, N, chunk_rows)[0]
        _lib.route_reset()
        gm, gv, gl = g.loo(chunk_rows=chunk_rows)
        assert _lib.route_count(_lib.ROUTE_LOO_CHUNK) == -(-N // rows)
        assert (_lib.route_count(_lib.ROUTE_TRSM_OPS) > 0) == cov_ops == (N == 1536)
        gk = np.empty(N)
        _lib.check(lib.gpx_gp_inv_diag(h, chunk_rows, _lib.dptr(gk)))
        print("%s N=%d %s chunk_rows=%d (%d rows a chunk)" % (kind, N, dtype, chunk_rows, rows))
        _check([("inv_Kxx_diag", gk, kii), ("loo_mean", gm, mean), ("loo_var", gv, var), ("log_p", gl, log_p)], ORACLE_TOL[dtype])
        np.testing.assert_allclose(g.loo_log_lh, log_p.sum(), **ORACLE_TOL[dtype])
        # the same call twice: the same bits (the second one is served from the handle's diagonal)
        again = g.loo(chunk_rows=chunk_rows)
        assert all(np.array_equal(a, b) for a, b in zip(again, (gm, gv, gl)))
        by_chunk[chunk_rows] = gk
    # two whole sweeps of the same factor values (the loop's last refit against one more): the same bits
    g.s = 2.0
    g.log_lh
    g.s = 1.0
    _lib.route_reset()
    resweep = g.loo(chunk_rows=512)
    assert _lib.route_count(_lib.ROUTE_LOO_CHUNK) == -(-N // 512)
    assert all(np.array_equal(a, b) for a, b in zip(resweep, (gm, gv, gl)))
    assert np.array_equal(g.inv_Kxx_diag, by_chunk[512])
    if dtype == "float64":
        for chunk_rows in (128, 512):
            assert np.abs(by_chunk[chunk_rows] - by_chunk[0]).max() <= 1e-10 * np.abs(kii).max()


# ---- 4. the operator route at N = 8192, two chunks of 4096 ----
def test_inv_diag_against_the_inverse_on_the_same_object():
    N, d = 8192, 3
    X, y, _ = orc.synth_inputs(N, d, 1)
    g = gp.GP(gp.GaussianKernel(1.0, 0.5 * np.sqrt(d)), X, y, s=1.0)
    g.log_lh
    _lib.route_reset()
    kii = g.inv_Kxx_diag
    assert _lib.route_count(_lib.ROUTE_LOO_CHUNK) == 2 and _lib.route_count(_lib.ROUTE_TRSM_OPS) == 2
    Ki = g.inv_Kxx
    err, bound = float(np.abs(kii - np.diag(Ki)).max()), 1e-10 * float(np.abs(Ki).max())
    print("inv_Kxx_diag vs diag(inv_Kxx): %.3e, bound %.3e" % (err, bound))
    assert err <= bound


# ---- 5. the finishing kernel alone ----
def test_d_loo_rows_kernel_masks_tails_and_alignment():
    """gpx_d_loo_rows alone: everything the kernel must not use holds NaN -- the padding at and beyond column n, and in
    every row the columns before its own first one -- with an aligned and a misaligned leading dimension, n that is no
    multiple of the vector width, chunks at the head and at the very end of the matrix."""
    lib = _lib.load()
    rng = np.random.RandomState(5)
    for dtype, npdt in ((_lib.F64, np.float64), (_lib.F32, np.float32)):
        for rows, n, ldx, c0 in ((130, 1003, 1008, 0), (130, 1003, 1008, 873), (130, 1003, 1005, 640), (130, 1003, 1005, 873),
                                 (128, 1024, 1024, 0), (128, 1024, 1024, 896), (128, 1024, 1025, 384)):
            Xh = np.full((rows, ldx), np.nan, dtype=npdt)
            for i in range(rows):
                Xh[i, c0 + i:n] = rng.randn(n - c0 - i)
            yv, av = rng.randn(rows).astype(npdt), rng.randn(rows).astype(npdt)
            ss = np.array([(Xh[i, c0 + i:n].astype(np.float64) ** 2).sum() for i in range(rows)])
            bufs = [ctypes.c_void_p() for _ in range(4)]
            for b, sz in zip(bufs, (Xh.nbytes, yv.nbytes, av.nbytes, 4 * rows * 8)):
                _lib.check(lib.gpx_malloc(ctypes.byref(b), sz))
            try:
                dX, dy, da, dout = bufs
                for dst, src in ((dX, Xh), (dy, yv), (da, av)):
                    _lib.check(lib.gpx_memcpy_h2d(dst, src.ctypes.data_as(ctypes.c_void_p), src.nbytes, None))
                o = [ctypes.c_void_p(dout.value + q * rows * 8) for q in range(4)]

                def run(fused):
                    out = np.empty((4, rows))
                    _lib.check(lib.gpx_memset(dout, 0xFF, out.nbytes, None))
                    if fused:
                        _lib.check(lib.gpx_d_loo_rows(dtype, dX, rows, n, ldx, c0, dy, da, o[0], o[1], o[2], o[3], None))
                    else:
                        _lib.check(lib.gpx_d_loo_rows(dtype, dX, rows, n, ldx, c0, None, None, o[0], None, None, None, None))
                    _lib.check(lib.gpx_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), dout, out.nbytes, None))
                    return out

                alone, fused = run(False), run(True)
                assert np.isfinite(alone[0]).all()
                np.testing.assert_allclose(alone[0], ss, rtol=1e-13, atol=0)
                assert np.array_equal(fused[0], alone[0]) and np.array_equal(run(True), fused)
                # division is correctly rounded and log within a few ulp: the per-point quantities from the kernel's own sums
                k, a, yy = fused[0], av.astype(np.float64), yv.astype(np.float64)
                mean, var, log_p = loo_from_diag(k, a, yy)
                np.testing.assert_allclose(fused[1], mean, rtol=0, atol=4 * _EPS * (np.abs(yy) + np.abs(a / k)).max())
                np.testing.assert_allclose(fused[2], var, rtol=4 * _EPS, atol=0)
                np.testing.assert_allclose(fused[3], log_p, rtol=0, atol=8 * _EPS * (np.abs(0.5 * np.log(k)) + 0.5 * a * a / k + 1).max())
            finally:
                for b in bufs:
                    lib.gpx_free(b)


# ---- 6. the handle keeps the diagonal for as long as the factor ----
def test_the_diagonal_is_swept_once_per_fit():
    x, y, make, (kii, mean, var, log_p) = _case("gaussian", 1000)
    g = gp.GP(make(), x, y, s=1.0)
    g.log_lh
    _lib.route_reset()
    # no output asked for: the sweep alone, and the property that follows finds the diagonal there
    assert _lib.load().gpx_gp_loo(g._fit_pd().handle, 0, None, None, None, None) == _lib.OK
    first = g.inv_Kxx_diag
    assert _lib.route_count(_lib.ROUTE_LOO_CHUNK) == 1
    _lib.route_reset()
    gm, gv, gl = g.loo()
    assert _lib.route_count(_lib.ROUTE_LOO_CHUNK) == 0
    assert np.array_equal(gv, 1.0 / first) or np.allclose(gv, 1.0 / first, rtol=4 * _EPS, atol=0)
    _check([("loo_mean", gm, mean), ("loo_var", gv, var), ("log_p", gl, log_p)], ORACLE_TOL["float64"])
    g.s = 0.5
    assert "inv_Kxx_diag" not in g._memoized and "loo_mean" not in g._memoized
    _lib.route_reset()
    second = g.inv_Kxx_diag
    assert _lib.route_count(_lib.ROUTE_LOO_CHUNK) == 1
    assert not np.allclose(second, first, rtol=1e-3)
    K = orc.OracleGP("gaussian", tuple(g.K.params), x, y, 0.5).Kxx
    _check([("inv_Kxx_diag after g.s = 0.5", second, loo_reference(K, y)[0])], ORACLE_TOL["float64"])


# ---- 7. a restored factor ----
def test_loo_after_checkpoint_is_bit_identical(tmp_path):
    x, y, make, _ = _case("gaussian", 1000)
    g = gp.GP(make(), x, y, s=1.0)
    before = g.loo()
    path = str(tmp_path / "fit.gpx")
    g.save_fitted(path)
    h = gp.GP.load_fitted(path)
    _lib.route_reset()
    after = h.loo()
    assert _lib.route_count(_lib.ROUTE_LOO_CHUNK) == 1
    assert all(np.array_equal(a, b) for a, b in zip(after, before))
    assert h.loo_log_lh == g.loo_log_lh and np.array_equal(h.inv_Kxx_diag, g.inv_Kxx_diag)


# ---- 8. kernels the path knows nothing about: it needs only the factor ----
def test_loo_plugin_kernel_and_ard():
    N, d = 1000, 3
    X, y, _ = orc.synth_inputs(N, d, 1)
    for g in (gp.GP(_PythonRBF(1.3, 0.9), X, y, s=1.0), gp.GP(gp.GaussianARDKernel(1.0, [0.7, 1.1, 1.6]), X, y, s=1.0)):
        kii, mean, var, log_p = loo_reference(g.Kxx, y)
        gm, gv, gl = g.loo()
        print(type(g.K).__name__)
        _check([("inv_Kxx_diag", g.inv_Kxx_diag, kii), ("loo_mean", gm, mean), ("loo_var", gv, var), ("log_p", gl, log_p)],
               ORACLE_TOL["float64"])
        np.testing.assert_allclose(g.loo_log_lh, log_p.sum(), **ORACLE_TOL["float64"])


# ---- 9. a fit that is not positive definite ----
def test_loo_of_a_fit_that_is_not_positive_definite():
    rec = load_golden("gp_nonpd.npz")
    h, w, s = rec["params"]
    g = gp.GP(gp.GaussianKernel(h, w), rec["x"], rec["y"], s=s)
    assert g.loo_log_lh == -np.inf
    for f in (lambda: g.loo_mean, lambda: g.loo_var, lambda: g.inv_Kxx_diag, g.loo):
        with pytest.raises(np.linalg.LinAlgError):
            f()
    out = np.empty(len(rec["y"]))
    lib = _lib.load()
    handle = g._fit().handle
    assert lib.gpx_gp_inv_diag(handle, 0, _lib.dptr(out)) == _lib.ERR_ARG and "not positive definite" in _lib.last_error()
    assert lib.gpx_gp_loo(handle, 0, _lib.dptr(out), None, None, None) == _lib.ERR_ARG
    assert lib.gpx_gp_inv_diag(handle, 100, _lib.dptr(out)) == _lib.ERR_ARG and "multiple of 128" in _lib.last_error()
