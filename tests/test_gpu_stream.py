"""GPU tests of the streamed reductions (csrc/gpx_stream.hip, DESIGN "Streamed reductions"): the fused posterior mean and
gpx_d_kmat_apply at one weight vector are two kernels from the same pieces and give the same bits, the dynamic-LDS limit of
every kernel on the path is set once per device for the largest d it takes (so any order of d in one process launches), and the refusals are the ones the three
separate kernels had.

Tolerances are the ones the project already holds these calls to: gpx_d_mean in fp64 rtol 1e-10, atol 1e-10 max|ref|
(tests/test_gpu_parity.py::test_fused_mean_device_api_vs_numpy; the kernel matrix in fp64 is held to the same), gpx_d_pred_grad
in fp64 ORACLE_TOL, and every fp32 result rtol 1e-2, atol 5e-3 max(1, max|ref|)
(tests/test_gpu_xgrad.py::test_range_of_d_is_the_mean_kernels)."""
import numpy as np
import pytest

from gaussian_processes_amd import _lib
from gaussian_processes_amd.device import DeviceBuffer, sync
from oracle import gp_oracle as orc
from test_gpu_paths import routes, _took          # noqa: F401  (routes: the fixture that forces a route of gpx_d_kmat_apply)
from test_gpu_xgrad import ORACLE_TOL, _pred_grad_direct

pytestmark = pytest.mark.gpu

NPDT = {"float64": np.float64, "float32": np.float32}
DTID = {"float64": _lib.F64, "float32": _lib.F32}
FAMILY = {"gaussian": (_lib.KERNEL_GAUSSIAN, np.array([1.3, 0.9])), "periodic": (_lib.KERNEL_PERIODIC, np.array([1.3, 0.8, 3.0]))}


@pytest.mark.parametrize("kernel", sorted(FAMILY))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m,d", [(600, 9, 3), (257, 1, 1)])
def test_mean_and_apply_at_one_vector_give_the_same_bits(n, m, d, dtype, kernel, routes):
    """gpx_d_mean(xo, x, alpha) and gpx_d_kmat_apply(S = 1, V = alpha) into a zeroed out: the same bits -- the two kernels form
    every kernel value through the same evaluator and add in the same order, and a change to one that is not made to the
    other shows here.  (600, 9, 3): several
    slices of the training set, a ragged last chunk, a d that does not divide 256; (257, 1, 1): one point, one lane of a
    second chunk.)"""
    T, rng, lib = NPDT[dtype], np.random.RandomState(n + m), _lib.load()
    kid, prm = FAMILY[kernel]
    x, xo, alpha = rng.uniform(-3, 3, (n, d)).astype(T), rng.uniform(-3, 3, (m, d)).astype(T), rng.randn(n).astype(T)
    dx, dxo, da = DeviceBuffer.from_host(x), DeviceBuffer.from_host(xo), DeviceBuffer.from_host(alpha)
    mean, applied = DeviceBuffer.from_host(np.full(m, -7.25, dtype=T)), DeviceBuffer((m,), T).zero()
    _lib.check(lib.gpx_d_mean(DTID[dtype], kid, dxo.ptr, m, dx.ptr, n, d, _lib.dptr(prm), da.ptr, mean.ptr, None))
    routes("fused")
    _lib.check(lib.gpx_d_kmat_apply(DTID[dtype], kid, dxo.ptr, m, dx.ptr, n, d, _lib.dptr(prm), da.ptr, n, 1, applied.ptr, m, None))
    sync()
    assert _took("fused")
    a, b = mean.to_host(), applied.to_host()
    assert np.abs(a).max() > 1e-3
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), np.abs(a.astype(np.float64) - b.astype(np.float64)).max()


def _tol(dtype, ref, f64):
    return f64 if dtype == "float64" else dict(rtol=1e-2, atol=5e-3 * max(1.0, float(np.abs(ref).max())))


# (the last two: a mid-size d above 48 KiB BEFORE the largest -- a limit set to the first call's own size would refuse the second)
@pytest.mark.parametrize("dtype,ds", [("float64", (47, 16, 47)), ("float32", (95, 3, 95)), ("float64", (30, 47)), ("float32", (60, 95))])
def test_large_d_in_any_order_in_one_process(dtype, ds):
    """The chunk of x needs more than 48 KiB of dynamic LDS from d = 24 (fp64) / 48 (fp32) on, and a kernel's limit is now set
    once per device instead of before every launch: the largest d, a small one and the largest again must all launch and
    agree with the numpy closed forms.  gpx_d_kmat refuses fp32 d = 95 as it always has (its own tile of column points: 95 x 260
    floats are more than 96 KiB; d = 94 is its largest), so there the refusal is asserted and the matrix is built at d = 94."""
    T, n, m, lib = NPDT[dtype], 257, 9, _lib.load()
    for d in ds:
        params = np.array([3.0, 3.0 * np.sqrt(d)])          # wide enough that every training point contributes
        X, _, Xo = orc.synth_inputs(n, d, m)
        X, Xo, alpha = X.astype(T), Xo.astype(T), np.random.RandomState(d).randn(n).astype(T)
        dx, dxo, da = DeviceBuffer.from_host(X), DeviceBuffer.from_host(Xo), DeviceBuffer.from_host(alpha)
        K = orc.kernel_matrix("gaussian", "K", Xo.astype(np.float64), X.astype(np.float64), tuple(params))
        # the mean
        out = DeviceBuffer((m,), T).zero()
        _lib.check(lib.gpx_d_mean(DTID[dtype], _lib.KERNEL_GAUSSIAN, dxo.ptr, m, dx.ptr, n, d, _lib.dptr(params), da.ptr, out.ptr, None))
        sync()
        ref = K @ alpha.astype(np.float64)
        assert np.abs(ref).max() > 1e-3
        np.testing.assert_allclose(out.to_host(), ref, **_tol(dtype, ref, dict(rtol=1e-10, atol=1e-10 * np.abs(ref).max())))
        # the input gradient
        rc, got, ref = _pred_grad_direct(dtype, d, m=m, n=n)
        assert rc == _lib.OK and np.abs(ref).max() > 1e-4
        np.testing.assert_allclose(got, ref, **_tol(dtype, ref, ORACLE_TOL))
        # the matrix
        dk, ldk = d, 272
        if dtype == "float32" and d == 95:
            Kd = DeviceBuffer((m, ldk), T).zero()
            rc = lib.gpx_d_kmat(DTID[dtype], _lib.KERNEL_GAUSSIAN, _lib.K, dxo.ptr, m, dx.ptr, n, d, _lib.dptr(params), 0.0, _lib.FULL,
                                Kd.ptr, ldk, None)
            assert rc == _lib.ERR_UNSUPPORTED and "kmat: d = 95 too large" in _lib.last_error()
            dk = 94
            X, Xo = np.ascontiguousarray(X[:, :dk]), np.ascontiguousarray(Xo[:, :dk])
            dx, dxo = DeviceBuffer.from_host(X), DeviceBuffer.from_host(Xo)
            K = orc.kernel_matrix("gaussian", "K", Xo.astype(np.float64), X.astype(np.float64), tuple(params))
        Kd = DeviceBuffer((m, ldk), T).zero()
        _lib.check(lib.gpx_d_kmat(DTID[dtype], _lib.KERNEL_GAUSSIAN, _lib.K, dxo.ptr, m, dx.ptr, n, dk, _lib.dptr(params), 0.0, _lib.FULL,
                                  Kd.ptr, ldk, None))
        sync()
        np.testing.assert_allclose(Kd.to_host()[:, :n], K, **_tol(dtype, K, dict(rtol=1e-10, atol=1e-10 * np.abs(K).max())))


def test_refusals_unchanged():
    """A chunk of x beyond 96 KiB of LDS (fp64 d = 48) and a periodic derivative member at d = 2 are refused with the texts
    the separate kernels had."""
    lib, n, m = _lib.load(), 300, 5
    X, _, Xo = orc.synth_inputs(n, 48, m)
    alpha = np.random.RandomState(0).randn(n)
    dx, dxo, da = DeviceBuffer.from_host(X), DeviceBuffer.from_host(Xo), DeviceBuffer.from_host(alpha)
    out, params = DeviceBuffer((m, 48)).zero(), np.array([3.0, 3.0 * np.sqrt(48)])
    rc = lib.gpx_d_mean(_lib.F64, _lib.KERNEL_GAUSSIAN, dxo.ptr, m, dx.ptr, n, 48, _lib.dptr(params), da.ptr, out.ptr, None)
    assert rc == _lib.ERR_UNSUPPORTED and _lib.last_error() == "mean: d = 48 too large"
    rc = lib.gpx_d_pred_grad(_lib.F64, _lib.KERNEL_GAUSSIAN, dxo.ptr, m, dx.ptr, n, 48, _lib.dptr(params), da.ptr, None, 0, 1.0,
                             out.ptr, None)
    assert rc == _lib.ERR_UNSUPPORTED and _lib.last_error() == "pred_grad: d = 48 too large"
    per = np.array([1.3, 0.8, 3.0])
    rc = lib.gpx_d_mean_member(_lib.F64, _lib.KERNEL_PERIODIC, _lib.DK_DH, dxo.ptr, m, dx.ptr, n, 2, _lib.dptr(per), da.ptr, out.ptr, None)
    assert rc == _lib.ERR_UNSUPPORTED and _lib.last_error() == "periodic derivative members need d == 1 (got 2)"
    rc = lib.gpx_d_kmat(_lib.F64, _lib.KERNEL_PERIODIC, _lib.DK_DH, dxo.ptr, m, dx.ptr, n, 2, _lib.dptr(per), 0.0, _lib.FULL,
                        DeviceBuffer((m, 304)).zero().ptr, 304, None)
    assert rc == _lib.ERR_UNSUPPORTED and _lib.last_error() == "periodic derivative members need d == 1 (got 2)"
    sync()
