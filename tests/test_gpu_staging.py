"""GPU tests of the handle's host-side plumbing: the one staging pair between host float64 and device arrays of the
handle's dtype (upload_f64 / download_f64, csrc/gpx_gp.hip), the row-chunk driver behind the plugin form of the
predictive variance, and the one read of the scalar block behind every status path.

The conversion is specified -- float64 -> dtype rounds to nearest, dtype -> float64 is exact -- so the first group asserts
equality, not closeness.  The plugin-kernel group uses ORACLE_TOL of tests/test_gpu_var.py (fp32: rtol 1e-2, atol 5e-3),
the bound test_var_plugin_kernel_through_var_from_K holds the same quantities to."""
import ctypes

import numpy as np
import pytest

from gaussian_processes_amd import _lib
import gaussian_processes_amd as gp
from oracle import gp_oracle as orc
from conftest import load_golden
from test_dist_gp_cpu import _PythonRBF
from test_gpu_var import ORACLE_TOL

pytestmark = pytest.mark.gpu

DTYPES = {"float64": (_lib.F64, np.float64), "float32": (_lib.F32, np.float32)}


class _Handle(object):
    """A raw gpx_gp_t of n points in d dimensions, destroyed on exit."""

    def __init__(self, dtype, n, d, kernel=_lib.KERNEL_GAUSSIAN):
        self.lib, self.h, self.n, self.d = _lib.load(), ctypes.c_void_p(), n, d
        self.code, self.np_dtype = DTYPES[dtype]
        _lib.check(self.lib.gpx_gp_create(ctypes.byref(self.h), self.code, kernel, n, d))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.gpx_gp_destroy(self.h)
        return False

    def device_matrix(self):
        """Rows and columns [0, n) of the handle's HBM matrix, in the handle's dtype."""
        A, lda = ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(self.lib.gpx_gp_device_ptrs(self.h, ctypes.byref(A), ctypes.byref(lda), None, None, None, None))
        es = np.dtype(self.np_dtype).itemsize
        assert lda.value == -(-self.n // 16) * 16
        out = np.empty((self.n, self.n), dtype=self.np_dtype)
        _lib.check(self.lib.gpx_memcpy2d_d2h(out.ctypes.data_as(ctypes.c_void_p), self.n * es, A, lda.value * es, self.n * es,
                                             self.n, None))
        return out


# ---- 1. upload and download are exact ----
# n = 1: the degenerate grid; n = 17: lda = 32, a pad behind every row; n = 300: a second 256-column block of the kernels
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [1, 17, 300])
def test_set_data_and_get_xy_round_trip_exactly(n, dtype):
    rng = np.random.RandomState(n)
    x, y = rng.standard_normal((n, 3)) * 3.0, rng.standard_normal(n)        # (not representable in fp32)
    with _Handle(dtype, n, 3) as g:
        _lib.check(g.lib.gpx_gp_set_data(g.h, _lib.dptr(x), _lib.dptr(y)))
        gx, gy = np.full((n, 3), np.nan), np.full(n, np.nan)
        _lib.check(g.lib.gpx_gp_get_xy(g.h, _lib.dptr(gx), _lib.dptr(gy)))
        assert np.array_equal(gx, x.astype(g.np_dtype).astype(np.float64))
        assert np.array_equal(gy, y.astype(g.np_dtype).astype(np.float64))
        if dtype == "float32":
            assert not np.array_equal(gx, x)                                    # (the conversion was there to be missed)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [1, 17, 300])
def test_set_K_with_a_host_leading_dimension_is_exact(n, dtype):
    rng = np.random.RandomState(100 + n)
    a = rng.standard_normal((n, n))
    K = a + a.T
    host = np.full((n, n + 3), 7.0)                                             # ld = n + 3: three columns that are not K's
    host[:, :n] = K
    with _Handle(dtype, n, 3) as g:
        _lib.check(g.lib.gpx_gp_set_K(g.h, _lib.dptr(host), n + 3))
        got = g.device_matrix()
        assert got.dtype == g.np_dtype
        assert np.array_equal(got, K.astype(g.np_dtype))
        if dtype == "float32":
            assert not np.array_equal(got.astype(np.float64), K)


# ---- 2. a ragged chunk through the plugin form ----
def test_ragged_chunk_through_the_plugin_form_fp32():
    n, m, d = 300, 130, 3
    X, y, Xo = orc.synth_inputs(n, d, m)
    kern, s = _PythonRBF(1.3, 0.9), 1.0
    A = kern.K(X, X) + s * s * np.eye(n)
    Kxox = np.ascontiguousarray(kern.K(Xo, X), dtype=np.float64)
    kdiag = np.ascontiguousarray(kern.diag(Xo), dtype=np.float64)
    sol = np.linalg.solve(A, Kxox.T)
    ref_var = kdiag - np.einsum("ij,ji->i", Kxox, sol)
    ref_mean = Kxox @ np.linalg.solve(A, y)
    Kxoxo = np.ascontiguousarray(kern.K(Xo[:3], Xo[:3]), dtype=np.float64)
    ref_cov = Kxoxo - Kxox[:3] @ sol[:, :3]
    with _Handle("float32", n, d) as g:
        lib, info = g.lib, ctypes.c_int(-1)
        _lib.check(lib.gpx_gp_set_data(g.h, _lib.dptr(np.ascontiguousarray(X)), _lib.dptr(np.ascontiguousarray(y))))
        _lib.check(lib.gpx_gp_set_K(g.h, _lib.dptr(np.ascontiguousarray(A)), n))
        _lib.check(lib.gpx_gp_fit(g.h, ctypes.byref(info)))
        assert info.value == 0
        var = np.full(m, np.nan)
        _lib.route_reset()
        _lib.check(lib.gpx_gp_var_from_K(g.h, _lib.dptr(Kxox), _lib.dptr(kdiag), m, 128, _lib.dptr(var)))
        assert _lib.route_count(_lib.ROUTE_VAR_CHUNK) == 2 == _lib.var_plan(_lib.F32, n, m, 128)[1]      # 128 rows, then 2
        np.testing.assert_allclose(var, ref_var, **ORACLE_TOL["float32"])
        mean, cov = np.full(3, np.nan), np.full((3, 3), np.nan)
        _lib.check(lib.gpx_gp_mean_from_K(g.h, _lib.dptr(Kxox), 3, _lib.dptr(mean)))
        _lib.check(lib.gpx_gp_cov_from_K(g.h, _lib.dptr(Kxox), _lib.dptr(Kxoxo), 3, _lib.dptr(cov)))
        np.testing.assert_allclose(mean, ref_mean[:3], **ORACLE_TOL["float32"])
        np.testing.assert_allclose(cov, ref_cov, **ORACLE_TOL["float32"])


# ---- 3. one status read, the same answers ----
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_status_paths_of_a_handle_that_is_not_positive_definite(dtype, tmp_path):
    n, d = 17, 3
    rng = np.random.RandomState(3)
    x, y = rng.standard_normal((n, d)), rng.standard_normal(n)
    with _Handle(dtype, n, d) as g:
        lib, info = g.lib, ctypes.c_int(-5)
        _lib.check(lib.gpx_gp_set_data(g.h, _lib.dptr(x), _lib.dptr(y)))
        _lib.check(lib.gpx_gp_set_K(g.h, _lib.dptr(-np.eye(n)), n))
        assert lib.gpx_gp_fit(g.h, ctypes.byref(info)) == _lib.OK and info.value == 1
        inf2, llh = ctypes.c_int(-5), ctypes.c_double(0.0)
        assert lib.gpx_gp_info(g.h, ctypes.byref(inf2)) == _lib.OK and inf2.value == 1
        assert lib.gpx_gp_log_lh(g.h, ctypes.byref(llh)) == _lib.OK and llh.value == -np.inf
        out = np.empty(n)
        assert lib.gpx_gp_inv_diag(g.h, 0, _lib.dptr(out)) == _lib.ERR_ARG
        assert "not positive definite (info = 1)" in _lib.last_error() and "diag(K^-1)" in _lib.last_error()
        assert lib.gpx_gp_loo(g.h, 0, _lib.dptr(out), None, None, None) == _lib.ERR_ARG
        assert "not positive definite (info = 1)" in _lib.last_error() and "diag(K^-1)" in _lib.last_error()
        h2, one = ctypes.c_void_p(), np.ones(1)
        rc = lib.gpx_gp_extend_from_K(g.h, _lib.dptr(np.zeros(d)), _lib.dptr(one), 1, _lib.dptr(np.zeros(n)), _lib.dptr(one),
                                      ctypes.byref(h2), ctypes.byref(info))
        assert rc == _lib.ERR_ARG and not h2.value
        assert "not positive definite (info = 1)" in _lib.last_error() and "to extend" in _lib.last_error()
        path = str(tmp_path / "nonpd.gpx").encode()
        assert lib.gpx_gp_save(g.h, path) == _lib.OK
        h3 = ctypes.c_void_p()
        assert lib.gpx_gp_load(ctypes.byref(h3), path) == _lib.OK
        try:
            inf3 = ctypes.c_int(-5)
            assert lib.gpx_gp_info(h3, ctypes.byref(inf3)) == _lib.OK and inf3.value == 1
            assert lib.gpx_gp_log_lh(h3, ctypes.byref(llh)) == _lib.OK and llh.value == -np.inf
        finally:
            lib.gpx_gp_destroy(h3)


def test_gradient_of_a_parameter_fit_that_is_not_positive_definite_is_nan():
    rec = load_golden("gp_nonpd.npz")
    hh, w, s = rec["params"]
    bad = gp.GP(gp.GaussianKernel(hh, w), rec["x"], rec["y"], s=s)
    st = bad._fit()
    assert st.info > 0
    out = np.zeros(3)
    assert _lib.load().gpx_gp_dloglh_dtheta(st.handle, _lib.dptr(out)) == _lib.OK
    assert np.isnan(out).all()
