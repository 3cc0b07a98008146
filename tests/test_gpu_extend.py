"""GPU tests of GP.extend (gpx_gp_extend, gpx_gp_extend_from_K) and of its two kernels (gpx_d_copy_lower,
gpx_d_schur_lower).

Tolerances are the project's own: ORACLE_TOL of tests/test_gpu_var.py against the oracle on the concatenated data (fp64 rtol
1e-7 / atol 1e-10, fp32 1e-2 / 5e-3) and 1e-10 * max|ref| between two fp64 device evaluations of one quantity, the bound of
tests/test_gpu_dist_cov.py.  The bordered factorisation itself, in numpy on the same inputs, stays within |dL| <= 3e-15 and
|dalpha| <= 4e-15 (fp32 arithmetic: 2e-6) of the direct one at every size below (cond(K) <= 650)."""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from conftest import load_golden
from test_dist_gp_cpu import _PythonRBF
from test_gpu_var import ORACLE_TOL
from _extend_helpers import DeviceBuffers, M_TEST, case, close, make_kernel

pytestmark = pytest.mark.gpu

_DTYPE_ID = {"float64": _lib.F64, "float32": _lib.F32}
_NP = {"float64": np.float64, "float32": np.float32}


def _handle_log_lh(g):
    """log_lh from the handle itself (the property is memoised on the host)."""
    out = ctypes.c_double(0.0)
    _lib.check(_lib.load().gpx_gp_log_lh(g._fit().handle, ctypes.byref(out)))
    return out.value


def _split(kind, n, k):
    x, y, xo, o = case(kind, n + k)
    return x[:n], y[:n], x[n:], y[n:], x, y, xo, o


# ---- 1. parity: every route and alignment case ----
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind", ["gaussian", "periodic", "ard"])
@pytest.mark.parametrize("n,k", [(999, 1), (999, 7), (1000, 9), (1536, 64), (1536, 200), (300, 300)])
def test_extend_parity(n, k, kind, dtype):
    x0, y0, xn, yn, x, y, xo, o = _split(kind, n, k)
    g = gp.GP(make_kernel(kind), x0, y0, s=1.0, dtype=dtype)
    L0 = g.Lxx
    _lib.route_reset()
    g2 = g.extend(xn, yn)
    assert _lib.route_count(_lib.ROUTE_EXTEND) == 1
    assert _lib.route_count(_lib.ROUTE_FIT_RIDE) + _lib.route_count(_lib.ROUTE_FIT_TWO_SOLVES) == 0
    assert (_lib.route_count(_lib.ROUTE_TRSM_OPS) > 0) == (n == 1536)
    assert isinstance(g2, gp.GP) and g2 is not g and g2.K is not g.K
    assert g2._n == n + k and g2.s == g.s and g2._dtype == g._dtype and np.array_equal(g2.K.params, g.K.params)
    assert np.array_equal(g2.x, x) and np.array_equal(g2.y, y)
    L2 = g2.Lxx
    assert np.array_equal(L2[:n, :n], L0)                   # the old rows are copied, not recomputed
    got = dict(Lxx=L2, inv_Kxx_y=g2.inv_Kxx_y, log_lh=g2.log_lh, mean=g2.mean(xo), var=g2.var(xo))
    ref = dict(Lxx=o.Lxx, inv_Kxx_y=o.inv_Kxx_y, log_lh=o.log_lh, mean=o.mean(o.xo), var=np.diag(o.cov(o.xo)))
    for name in ("Lxx", "inv_Kxx_y", "log_lh", "mean", "var"):
        print("%s vs oracle: err %.3e" % (name, float(np.abs(np.asarray(got[name]) - ref[name]).max())))
        np.testing.assert_allclose(got[name], ref[name], err_msg=name, **ORACLE_TOL[dtype])
    assert got["mean"].shape == (M_TEST,)
    if dtype == "float64":
        r = gp.GP(make_kernel(kind), x, y, s=1.0)
        for name, val in (("Lxx", r.Lxx), ("inv_Kxx_y", r.inv_Kxx_y), ("log_lh", r.log_lh), ("mean", r.mean(xo)), ("var", r.var(xo))):
            print(name)
            close(got[name], val)
    # the source is what it was
    assert np.array_equal(g.x, x0) and g._n == n
    assert np.array_equal(L0, _fresh_L(g))


def _fresh_L(g):
    out = np.empty((g._n, g._n))
    _lib.check(_lib.load().gpx_gp_get_Lxx(g._dev.handle, _lib.dptr(out), g._n))
    return out


# ---- 2. the loop: one point at a time ----
def test_extend_loop_of_single_points():
    n, steps = 500, 5
    x0, y0, xn, yn, x, y, xo, o = _split("gaussian", n, steps)
    cur = gp.GP(make_kernel("gaussian"), x0, y0, s=1.0)
    for i in range(steps):
        before = (_handle_log_lh(cur), cur.mean(xo))
        nxt = cur.extend(xn[i:i + 1], yn[i:i + 1])
        assert _handle_log_lh(cur) == before[0] and np.array_equal(cur.mean(xo), before[1])
        cur = nxt
    assert cur._n == n + steps
    np.testing.assert_allclose(cur.log_lh, o.log_lh, **ORACLE_TOL["float64"])
    np.testing.assert_allclose(cur.inv_Kxx_y, o.inv_Kxx_y, **ORACLE_TOL["float64"])
    r = gp.GP(make_kernel("gaussian"), x, y, s=1.0)
    close(cur.log_lh, r.log_lh)
    close(cur.inv_Kxx_y, r.inv_Kxx_y)
    for a, b in zip(cur.predict_grad(xo), r.predict_grad(xo)):
        close(a, b)


# ---- 3. repeatability ----
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_extend_is_bitwise_repeatable(dtype):
    x0, y0, xn, yn = _split("gaussian", 1536, 64)[:4]
    g = gp.GP(make_kernel("gaussian"), x0, y0, s=1.0, dtype=dtype)
    a, b = g.extend(xn, yn), g.extend(xn, yn)
    assert np.array_equal(a.Lxx, b.Lxx)
    assert np.array_equal(a.inv_Kxx_y, b.inv_Kxx_y)
    assert a.log_lh == b.log_lh


# ---- 4. an ordinary handle afterwards ----
def test_extended_gp_is_an_ordinary_gp(tmp_path):
    n, k, k2 = 999, 7, 9
    x, y, xo, _ = case("gaussian", n + k + k2)
    g2 = gp.GP(make_kernel("gaussian"), x[:n], y[:n], s=1.0).extend(x[n:n + k], y[n:n + k])
    r = gp.GP(make_kernel("gaussian"), x[:n + k], y[:n + k], s=1.0)
    for a, b in zip(g2.loo(), r.loo()):
        close(a, b)
    close(g2.inv_Kxx_diag, r.inv_Kxx_diag)
    close(g2.cov(xo), r.cov(xo))
    np.testing.assert_allclose(g2.dloglh_dtheta, r.dloglh_dtheta, **ORACLE_TOL["float64"])
    path = tmp_path / "extended.gpx"
    g2.save_fitted(path)
    back = gp.GP.load_fitted(path)
    assert back._n == n + k and back.log_lh == g2.log_lh
    assert np.array_equal(back.inv_Kxx_y, g2.inv_Kxx_y) and np.array_equal(back.Lxx, g2.Lxx)
    g3 = g2.extend(x[n + k:], y[n + k:])
    r3 = gp.GP(make_kernel("gaussian"), x, y, s=1.0)
    close(g3.Lxx, r3.Lxx)
    close(g3.inv_Kxx_y, r3.inv_Kxx_y)
    close(g3.log_lh, r3.log_lh)
    close(g3.mean(xo), r3.mean(xo))


# ---- 5. a plugin kernel ----
def test_extend_plugin_kernel():
    n, k, h, ell = 300, 7, 1.3, 0.9
    x0, y0, xn, yn, x, y, xo, _ = _split("gaussian", n, k)
    p = gp.GP(_PythonRBF(h, ell), x0, y0, s=1.0)
    _lib.route_reset()
    p2 = p.extend(xn, yn)
    assert _lib.route_count(_lib.ROUTE_EXTEND) == 1
    assert isinstance(p2.K, _PythonRBF) and p2.K is not p.K
    # the built-in Gaussian family is h^2 / (w sqrt(2 pi)) exp(-r^2 / (2 w^2))
    q2 = gp.GP(gp.GaussianKernel(h * np.sqrt(ell * np.sqrt(2 * np.pi)), ell), x0, y0, s=1.0).extend(xn, yn)
    close(p2.Lxx, q2.Lxx)
    close(p2.inv_Kxx_y, q2.inv_Kxx_y)
    close(p2.log_lh, q2.log_lh)
    close(p2.mean(xo), q2.mean(xo))
    close(p2.var(xo), q2.var(xo))


# ---- 6. not positive definite: status paths only ----
class _BrokenRBF(_PythonRBF):
    """K(a, a) of exactly three points is -2 I: with s = 1 the new diagonal block is -I."""

    def K(self, x1, x2, out=None):
        if len(x1) == 3 and len(x2) == 3:
            return -2.0 * np.eye(3)
        return _PythonRBF.K(self, x1, x2, out)


def test_extend_not_positive_definite():
    n, k = 200, 3
    x0, y0, xn, yn = _split("gaussian", n, k)[:4]
    lib = _lib.load()
    g = gp.GP(make_kernel("gaussian"), x0, y0, s=1.0)
    st = g._fit_pd()
    Kno = np.ascontiguousarray(g.K(xn, x0), dtype=np.float64)
    Knn = -np.eye(k)
    h, info = ctypes.c_void_p(), ctypes.c_int(-5)
    rc = lib.gpx_gp_extend_from_K(st.handle, _lib.dptr(np.ascontiguousarray(xn)), _lib.dptr(np.ascontiguousarray(yn)), k,
                                  _lib.dptr(Kno), _lib.dptr(Knn), ctypes.byref(h), ctypes.byref(info))
    try:
        assert rc == _lib.OK and info.value == n + 1 and h.value
        llh, inf2 = ctypes.c_double(0.0), ctypes.c_int(0)
        assert lib.gpx_gp_log_lh(h, ctypes.byref(llh)) == _lib.OK and llh.value == -np.inf
        assert lib.gpx_gp_info(h, ctypes.byref(inf2)) == _lib.OK and inf2.value == n + 1
    finally:
        lib.gpx_gp_destroy(h)
    # the same through a plugin kernel
    p2 = gp.GP(_BrokenRBF(1.3, 0.9), x0, y0, s=1.0).extend(xn, yn)
    assert p2.log_lh == -np.inf
    with pytest.raises(np.linalg.LinAlgError):
        p2.Lxx
    with pytest.raises(np.linalg.LinAlgError):
        p2.mean(xn)
    # a source whose own fit is not positive definite
    rec = load_golden("gp_nonpd.npz")
    hh, w, s = rec["params"]
    bad = gp.GP(gp.GaussianKernel(hh, w), rec["x"], rec["y"], s=s)
    with pytest.raises(np.linalg.LinAlgError):
        bad.extend(np.array([0.5]), np.array([0.0]))
    one = np.array([0.5])
    h2 = ctypes.c_void_p()
    rc = lib.gpx_gp_extend(bad._fit().handle, _lib.dptr(one), _lib.dptr(one), 1, ctypes.byref(h2), ctypes.byref(info))
    assert rc == _lib.ERR_ARG and not h2.value and "not positive definite" in _lib.last_error()
    assert bad.log_lh == -np.inf                             # ... and is what it was


# ---- 7. non-finite input ----
def test_extend_non_finite_input():
    n, k = 200, 3
    x0, y0, xn, yn = _split("gaussian", n, k)[:4]
    g = gp.GP(make_kernel("gaussian"), x0, y0, s=1.0)
    llh = g.log_lh
    bad_x = xn.copy()
    bad_x[1, 2] = np.nan
    with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
        g.extend(bad_x, yn)
    for bad in (np.nan, np.inf):
        bad_y = yn.copy()
        bad_y[0] = bad
        g2 = g.extend(xn, bad_y)
        with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
            g2.log_lh
    assert _handle_log_lh(g) == llh


# ---- 8. gpx_d_copy_lower ----
def _check_copy_lower(dtype, n, lds, ldd, offset):
    T, vec = _NP[dtype], 16 // np.dtype(_NP[dtype]).itemsize
    rng = np.random.RandomState(n + ldd)
    src = rng.standard_normal((n, lds)).astype(T)
    sentinel = T(-7.25)
    dst0 = np.full(n * ldd + offset, sentinel, dtype=T)
    with DeviceBuffers() as dev:
        ds, dd = dev.put(src), dev.put(dst0)
        dptr = ctypes.c_void_p(dd.value + offset * src.itemsize)
        _lib.check(dev.lib.gpx_d_copy_lower(_DTYPE_ID[dtype], ds, lds, dptr, ldd, n, None))
        flat = dev.get(dd, dst0)
    assert np.array_equal(flat[:offset], dst0[:offset])
    got = flat[offset:].reshape(n, ldd)
    i, j = np.arange(n)[:, None], np.arange(ldd)[None, :]
    lower = (j <= i)[:, :n]
    assert np.array_equal(got[:, :n][lower].view(np.uint8), src[:, :n][lower].view(np.uint8))      # bit for bit
    right = j >= (i // vec + 1) * vec                        # right of the 16-byte vector that holds the diagonal
    assert np.all(got[right] == sentinel)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("lds,ldd", [(144, 144), (144, 160)])
@pytest.mark.parametrize("n", [1, 17, 130])
def test_copy_lower(n, lds, ldd, dtype):
    _check_copy_lower(dtype, n, lds, ldd, 0)


@pytest.mark.parametrize("n", [1, 17, 130])
def test_copy_lower_unaligned_destination(n):
    _check_copy_lower("float64", n, 144, 160, 1)


# ---- 9. gpx_d_schur_lower ----
def _run_schur(dev, dtype, B, S0, k, n, ldb, lds):
    db, ds = dev.put(B), dev.put(S0)
    _lib.check(dev.lib.gpx_d_schur_lower(_DTYPE_ID[dtype], db, k, n, ldb, ds, lds, None))
    return dev.get(ds, S0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("k,n,ldb", [(1, 1, 16), (1, 1000, 1008), (7, 999, 1008), (64, 4097, 4112), (200, 1536, 1536), (7, 999, 999),
                                     (200, 200, 208), (130, 256, 256)],
                         ids=["1x1", "1x1000", "7x999", "64x4097", "200x1536", "7x999_unaligned", "200x200_one_slice", "130x256_one_slice"])
def test_schur_lower(k, n, ldb, dtype):
    """|got - ref| <= 2 (n + 1) eps (|S0| + sum_c |B_ic B_jc|) elementwise: the inner-product bound gamma_(n+1) with a factor
    2; the reference is numpy float64 on the same rounded inputs."""
    T = _NP[dtype]
    eps = float(np.finfo(T).eps)
    rng = np.random.RandomState(k * 31 + n)
    lds = -(-k // 16) * 16
    B = np.full((k, ldb), np.nan, dtype=T)                   # the padding beyond n is never read
    B[:, :n] = rng.standard_normal((k, n)).astype(T)
    sentinel = T(7.25)
    S0 = np.full((k, lds), sentinel, dtype=T)
    low = np.tril_indices(k)
    S0[low] = (rng.standard_normal(len(low[0])) * np.sqrt(n)).astype(T)
    with DeviceBuffers() as dev:
        got = _run_schur(dev, dtype, B, S0, k, n, ldb, lds)
        again = _run_schur(dev, dtype, B, S0, k, n, ldb, lds)
    Bd = B[:, :n].astype(np.float64)
    ref = S0[:, :k].astype(np.float64) - Bd @ Bd.T
    bound = 2.0 * (n + 1) * eps * (np.abs(S0[:, :k].astype(np.float64)) + np.abs(Bd) @ np.abs(Bd).T)
    err = np.abs(got[:, :k].astype(np.float64) - ref)
    print("schur_lower: max err / bound %.3e" % float((err[low] / bound[low]).max()))
    assert np.all(err[low] <= bound[low])
    upper = np.ones((k, lds), dtype=bool)
    upper[low] = False
    assert np.all(got[upper] == sentinel)                    # the strict upper triangle and the padding are untouched
    assert np.array_equal(got, again)
