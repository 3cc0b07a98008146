"""GPU tests of GP.remove (gpx_gp_remove) and of its primitive (gpx_d_chol_delete).

Tolerances are the project's own: ORACLE_TOL of tests/test_gpu_var.py against the oracle on the kept rows (fp64 rtol 1e-7 /
atol 1e-10, fp32 1e-2 / 5e-3) and 1e-10 * max|ref| between two fp64 evaluations of one quantity, the bound of
tests/test_gpu_dist_cov.py.  The deletion itself, in numpy on the same inputs, stays within 1.5e-15 max|L| of the direct
factorisation of the reduced matrix at every size below (cond(K) <= 570; fp32 arithmetic: 2.2e-7)."""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from conftest import load_golden
from test_dist_gp_cpu import _PythonRBF
from test_gpu_var import ORACLE_TOL
from _extend_helpers import DeviceBuffers, M_TEST, case, close, make_kernel
from _remove_helpers import HANDLE_IDS, HANDLE_SHAPES, SHAPE_IDS, SHAPES, cholesky_delete, kept_case

pytestmark = pytest.mark.gpu

_DTYPE_ID = {"float64": _lib.F64, "float32": _lib.F32}
_NP = {"float64": np.float64, "float32": np.float32}
_FIVE = ("Lxx", "inv_Kxx_y", "log_lh", "mean", "var")


def _idx_ptr(idx):
    a = np.ascontiguousarray(idx, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _handle_log_lh(g):
    """log_lh from the handle itself (the property is memoised on the host)."""
    out = ctypes.c_double(0.0)
    _lib.check(_lib.load().gpx_gp_log_lh(g._fit().handle, ctypes.byref(out)))
    return out.value


def _fresh_L(g):
    out = np.empty((g._n, g._n))
    _lib.check(_lib.load().gpx_gp_get_Lxx(g._dev.handle, _lib.dptr(out), g._n))
    return out


# ---- 1. the primitive against its numpy restatement ----
_DELETED = {}


def _deleted(n, idx, dtype):
    """(L in the dtype, cholesky_delete of exactly that L in float64): once per (n, idx, dtype)."""
    key = (n, tuple(idx), dtype)
    if key not in _DELETED:
        L = np.tril(case("gaussian", n)[3].Lxx).astype(_NP[dtype])
        _DELETED[key] = (L, cholesky_delete(L.astype(np.float64), idx))
    return _DELETED[key]


def _run_delete(dev, dtype, L, n, ldl, idx, ldo, off_l, off_o):
    """gpx_d_chol_delete on a factor at pitch ldl, `off_l` elements into its block, into a sentinel-filled block at pitch ldo,
    `off_o` elements in; returns (out block after, out block before, source block after, source block before)."""
    T, k = _NP[dtype], len(idx)
    src0 = np.full(n * ldl + off_l, T(3.5), dtype=T)
    src = src0[off_l:].reshape(n, ldl)
    src[:, :n] = np.triu(np.full((n, n), np.nan, dtype=T), 1) + L      # NaN above the diagonal: never read
    out0 = np.full((n - k) * ldo + off_o, T(-7.25), dtype=T)
    ds, do = dev.put(src0), dev.put(out0)
    a, p = _idx_ptr(idx)
    _lib.check(dev.lib.gpx_d_chol_delete(_DTYPE_ID[dtype], ctypes.c_void_p(ds.value + off_l * src0.itemsize), n, ldl, p, k,
                                         ctypes.c_void_p(do.value + off_o * src0.itemsize), ldo, None))
    return dev.get(do, out0), out0, dev.get(ds, src0), src0


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("layout", ["aligned", "unaligned"])
@pytest.mark.parametrize("n,idx", [(n, idx) for n, idx, _ in SHAPES], ids=SHAPE_IDS)
def test_chol_delete(n, idx, layout, dtype):
    k = len(idx)
    L, ref = _deleted(n, idx, dtype)
    if layout == "aligned":
        ldl, ldo, off_l, off_o = -(-n // 16) * 16, -(-(n - k) // 16) * 16, 0, 0
    else:
        ldl, ldo, off_l, off_o = n + 3, n - k + 5, 1, 3
    with DeviceBuffers() as dev:
        flat, out0, src_after, src0 = _run_delete(dev, dtype, L, n, ldl, idx, ldo, off_l, off_o)
    assert np.array_equal(src_after.view(np.uint8), src0.view(np.uint8))                  # the source is only read
    assert np.array_equal(flat[:off_o], out0[:off_o])
    got = flat[off_o:].reshape(n - k, ldo)
    low = np.tril_indices(n - k)
    err = float(np.abs(got[:, :n - k][low].astype(np.float64) - ref[low]).max())
    print("chol_delete vs numpy: err %.3e, max|ref| %.3e" % (err, float(np.abs(ref).max())))
    if dtype == "float64":
        assert err <= 1e-10 * np.abs(ref).max()
    else:
        np.testing.assert_allclose(got[:, :n - k][low], ref[low], **ORACLE_TOL[dtype])
    upper = np.ones((n - k, ldo), dtype=bool)
    upper[low] = False
    assert np.all(got[upper] == _NP[dtype](-7.25))           # the strict upper triangle and the padding are untouched
    r0 = min(idx)
    keep = np.setdiff1d(np.arange(n), idx)
    lead = np.tril(np.ones((n - k, n - k), dtype=bool))[:, :r0]
    assert np.array_equal(got[:, :r0][lead], L[keep][:, :r0][lead])                     # copied, not recomputed


def test_chol_delete_refuses_bad_arguments():
    n = 8
    L = np.tril(case("gaussian", 65)[3].Lxx[:n, :n]).copy()
    lib = _lib.load()
    with DeviceBuffers() as dev:
        dl, do = dev.put(L), dev.put(np.zeros((n, n)))
        for idx, ldl, ldo, out in [([3, 2], n, n, do), ([2, 2], n, n, do), ([8], n, n, do), ([-1], n, n, do),
                                   (list(range(n)), n, n, do), ([2], n - 1, n, do), ([2], n, n - 2, do), ([2], n, n, dl)]:
            a, p = _idx_ptr(idx)
            assert lib.gpx_d_chol_delete(_lib.F64, dl, n, ldl, p, len(idx), out, ldo, None) == _lib.ERR_ARG, idx
        assert lib.gpx_d_chol_delete(_lib.F64, dl, n, n, None, 1, do, n, None) == _lib.ERR_ARG
        assert lib.gpx_d_chol_delete(_lib.F64, dl, n, n, _idx_ptr([1])[1], 0, do, n, None) == _lib.ERR_ARG


# ---- 2. parity of g.remove(idx) ----
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind", ["gaussian", "periodic", "ard"])
@pytest.mark.parametrize("n,idx", HANDLE_SHAPES, ids=HANDLE_IDS)
def test_remove_parity(n, idx, kind, dtype):
    x, y, xo, o = kept_case(kind, n, idx)
    xk, yk = np.delete(x, idx, axis=0), np.delete(y, idx)
    g = gp.GP(make_kernel(kind), x, y, s=1.0, dtype=dtype)
    L0, llh0 = g.Lxx, _handle_log_lh(g)
    _lib.route_reset()
    g2 = g.remove(idx)
    assert _lib.route_count(_lib.ROUTE_REMOVE) == 1
    assert _lib.route_count(_lib.ROUTE_FIT_RIDE) + _lib.route_count(_lib.ROUTE_FIT_TWO_SOLVES) == 0
    assert isinstance(g2, gp.GP) and g2 is not g and g2.K is not g.K
    assert g2._n == n - len(idx) and g2.s == g.s and g2._dtype == g._dtype and np.array_equal(g2.K.params, g.K.params)
    assert np.array_equal(g2.x, xk) and np.array_equal(g2.y, yk)
    L2 = g2.Lxx
    r0 = min(idx)
    keep = np.setdiff1d(np.arange(n), idx)
    assert np.array_equal(L2[:, :r0], L0[keep][:, :r0])      # rows and columns below min(idx) are copied, not recomputed
    got = dict(Lxx=L2, inv_Kxx_y=g2.inv_Kxx_y, log_lh=g2.log_lh, mean=g2.mean(xo), var=g2.var(xo))
    ref = dict(Lxx=o.Lxx, inv_Kxx_y=o.inv_Kxx_y, log_lh=o.log_lh, mean=o.mean(o.xo), var=np.diag(o.cov(o.xo)))
    for name in _FIVE:
        print("%s vs oracle: err %.3e" % (name, float(np.abs(np.asarray(got[name]) - ref[name]).max())))
        np.testing.assert_allclose(got[name], ref[name], err_msg=name, **ORACLE_TOL[dtype])
    assert got["mean"].shape == (M_TEST,)
    if dtype == "float64":
        r = gp.GP(make_kernel(kind), xk, yk, s=1.0)
        for name, val in (("Lxx", r.Lxx), ("inv_Kxx_y", r.inv_Kxx_y), ("log_lh", r.log_lh), ("mean", r.mean(xo)), ("var", r.var(xo))):
            print(name)
            close(got[name], val)
    # the source is what it was
    assert np.array_equal(g.x, x) and g._n == n
    assert np.array_equal(L0, _fresh_L(g)) and _handle_log_lh(g) == llh0


def test_remove_accepts_masks_negative_and_unsorted_indices():
    n = 300
    x, y, xo, _ = case("gaussian", n)
    g = gp.GP(make_kernel("gaussian"), x, y, s=1.0)
    ref = g.remove([5, 77, 299])
    mask = np.zeros(n, dtype=bool)
    mask[[5, 77, 299]] = True
    for idx in ([-1, 77, 5], mask, np.array([77, 299, 5], dtype=np.int32)):
        other = g.remove(idx)
        assert np.array_equal(other.Lxx, ref.Lxx) and np.array_equal(other.x, ref.x) and other.log_lh == ref.log_lh
    one = g.remove(-300)
    assert one._n == n - 1 and np.array_equal(one.x, x[1:])


# ---- 3. an independent check: leave-one-out ----
def test_remove_one_point_is_leave_one_out():
    n = 500
    x, y, xo, _ = case("gaussian", n)
    g = gp.GP(make_kernel("gaussian"), x, y, s=1.0)
    for i in (0, 64, n - 1):
        g2 = g.remove(i)
        np.testing.assert_allclose(g2.mean(x[i:i + 1])[0], g.loo_mean[i], **ORACLE_TOL["float64"])
        np.testing.assert_allclose(g2.var(x[i:i + 1], noise=True)[0], g.loo_var[i], **ORACLE_TOL["float64"])


# ---- 4. the sliding window ----
def test_sliding_window():
    n, steps = 500, 5
    x, y, xo, _ = case("gaussian", n + steps)
    g = gp.GP(make_kernel("gaussian"), x[:n], y[:n], s=1.0)
    for t in range(steps):
        g = g.extend(x[n + t:n + t + 1], y[n + t:n + t + 1]).remove(0)
    assert g._n == n and np.array_equal(g.x, x[steps:]) and np.array_equal(g.y, y[steps:])
    r = gp.GP(make_kernel("gaussian"), x[steps:], y[steps:], s=1.0)
    close(g.inv_Kxx_y, r.inv_Kxx_y)
    close(g.log_lh, r.log_lh)
    for a, b in zip(g.predict_grad(xo), r.predict_grad(xo)):
        close(a, b)


# ---- 5. joint = sequential; repeatability ----
def test_joint_removal_equals_sequential():
    x, y, xo, _ = case("gaussian", 500)
    g = gp.GP(make_kernel("gaussian"), x, y, s=1.0)
    a, b = 40, 333
    joint, seq = g.remove([a, b]), g.remove(a).remove(b - 1)
    assert np.array_equal(joint.x, seq.x)
    for name in ("Lxx", "inv_Kxx_y", "log_lh"):
        close(getattr(joint, name), getattr(seq, name))
    close(joint.mean(xo), seq.mean(xo))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_remove_is_bitwise_repeatable(dtype):
    n, idx = HANDLE_SHAPES[0]
    x, y, xo, _ = case("gaussian", n)
    g = gp.GP(make_kernel("gaussian"), x, y, s=1.0, dtype=dtype)
    a, b = g.remove(idx), g.remove(idx)
    assert np.array_equal(a.Lxx, b.Lxx)
    assert np.array_equal(a.inv_Kxx_y, b.inv_Kxx_y)
    assert a.log_lh == b.log_lh


# ---- 6. an ordinary handle afterwards ----
def test_shrunk_gp_is_an_ordinary_gp(tmp_path):
    n, idx, k2 = 520, HANDLE_SHAPES[0][1], 9
    assert HANDLE_SHAPES[0][0] == n
    x, y, xo, _ = case("gaussian", n)
    m = n - k2
    keep = np.setdiff1d(np.arange(m), idx[:-1])              # (the last index, n - 1, lies in the part appended below)
    g2 = gp.GP(make_kernel("gaussian"), x[:m], y[:m], s=1.0).remove(idx[:-1])
    r = gp.GP(make_kernel("gaussian"), x[keep], y[keep], s=1.0)
    for a, b in zip(g2.loo(), r.loo()):
        close(a, b)
    close(g2.sample(xo, size=3, seed=5), r.sample(xo, size=3, seed=5))
    path = tmp_path / "shrunk.gpx"
    g2.save_fitted(path)
    back = gp.GP.load_fitted(path)
    assert back._n == len(keep) and back.log_lh == g2.log_lh
    assert np.array_equal(back.inv_Kxx_y, g2.inv_Kxx_y) and np.array_equal(back.Lxx, g2.Lxx)
    g3 = g2.extend(x[m:], y[m:])
    r3 = gp.GP(make_kernel("gaussian"), np.concatenate([x[keep], x[m:]]), np.concatenate([y[keep], y[m:]]), s=1.0)
    close(g3.Lxx, r3.Lxx)
    close(g3.inv_Kxx_y, r3.inv_Kxx_y)
    close(g3.log_lh, r3.log_lh)
    close(g3.mean(xo), r3.mean(xo))


# ---- 7. a plugin kernel ----
def test_remove_plugin_kernel():
    n, h, ell, idx = 300, 1.3, 0.9, [0, 31, 32, 150, 299]
    x, y, xo, _ = case("gaussian", n)
    p = gp.GP(_PythonRBF(h, ell), x, y, s=1.0)
    _lib.route_reset()
    p2 = p.remove(idx)
    assert _lib.route_count(_lib.ROUTE_REMOVE) == 1
    assert isinstance(p2.K, _PythonRBF) and p2.K is not p.K
    # the built-in Gaussian family is h^2 / (w sqrt(2 pi)) exp(-r^2 / (2 w^2))
    q2 = gp.GP(_PythonRBF(h, ell), np.delete(x, idx, axis=0), np.delete(y, idx), s=1.0)
    close(p2.Lxx, q2.Lxx)
    close(p2.inv_Kxx_y, q2.inv_Kxx_y)
    close(p2.log_lh, q2.log_lh)
    close(p2.mean(xo), q2.mean(xo))
    close(p2.var(xo), q2.var(xo))


# ---- 8. not positive definite: status paths only ----
def test_remove_from_a_source_that_is_not_positive_definite():
    rec = load_golden("gp_nonpd.npz")
    hh, w, s = rec["params"]
    bad = gp.GP(gp.GaussianKernel(hh, w), rec["x"], rec["y"], s=s)
    with pytest.raises(np.linalg.LinAlgError):
        bad.remove(0)
    lib = _lib.load()
    h2, info = ctypes.c_void_p(), ctypes.c_int(0)
    rc = lib.gpx_gp_remove(bad._fit().handle, _idx_ptr([0])[1], 1, ctypes.byref(h2), ctypes.byref(info))
    assert rc == _lib.ERR_ARG and not h2.value and "not positive definite" in _lib.last_error()     # no handle was left behind
    assert bad.log_lh == -np.inf                             # ... and the source is what it was


def test_remove_timing_stages():
    x, y, xo, _ = case("gaussian", 500)
    t = gp.GP(make_kernel("gaussian"), x, y, s=1.0).remove([3, 400]).fit_timing()
    # stage 0 lies between two events recorded back to back: no work, far below half a millisecond
    assert abs(t["kernel_build"]) < 0.5 and t["potrf"] > 0 and t["solve"] > 0 and t["total"] >= t["potrf"]
