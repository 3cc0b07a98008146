"""GPU tests of PosteriorPaths.grad / value_and_grad: the two device primitives (gpx_d_rff_features_grad,
gpx_d_kmat_apply_grad), gpx_paths_grad against the numpy restatement of a path's gradient (tests/_paths_grad_helpers.py) and
against central differences of the device's own values, and the semantics (chunking, buffers, prefix property, independence
of the source GP, ARD at equal widths).

Bounds.  u = 2^-53, eps = the dtype's machine epsilon.
  features' derivative   the bound of tests/test_gpu_paths.py's feature test times |Omega[f, k] / div_k|:
            ((d + 2) u sum_k |omega_fk p_ik| scale + 4 u scale) |omega_fk / div_k|; fp32: + 2^-24 |ref|, the store.
  kmat_apply_grad against float64 numpy with K from gpx_d_kmat in the same dtype and the differences formed in that dtype (the
            device forms the same kernel values and the same differences: only the accumulation and the last rounding remain):
            (n + 4) u mag + eps |ref + out0|,  mag[s, i, k] = 1 / (w^2 div_k) sum_j |V_sj K_ij (a_ik - x_jk)|  -- f64 sums of n
            terms, the product k V, the constant, the division and the += into a NON-ZERO block, one rounding to dtype.
  paths.grad against the restatement: the project's C_COND cond(Kxx) eps scale_g (tests/_paths_grad_helpers.py: grad_ref)."""
import ctypes
import gc

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from _extend_helpers import DeviceBuffers
from _paths_grad_helpers import features_grad_ref, grad_ref
from _sample_helpers import C_COND
from test_gpu_paths import _data, _gp, _kernel, _xo

pytestmark = pytest.mark.gpu

_DTYPE_ID = {"float64": _lib.F64, "float32": _lib.F32}
_NP = {"float64": np.float64, "float32": np.float32}
U = 2.0 ** -53


def _eps(dtype):
    return float(np.finfo(_NP[dtype]).eps)


# ---- 1. the derivative of the feature map ----
@pytest.mark.parametrize("div", [False, True], ids=["plain", "col_div"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("m,d,F,ld", [(1, 1, 1, 16), (7, 3, 5, 16), (130, 3, 130, 272), (33, 7, 64, 128)])
def test_rff_features_grad_matches_the_restatement(m, d, F, ld, dtype, div):
    T, rng, scale, sentinel = _NP[dtype], np.random.RandomState(m + F), 0.37, -7.25
    pts = rng.uniform(-10, 10, (m, d)).astype(T)
    omega = rng.randn(F, d) / 0.7
    w = rng.uniform(0.5, 2.0, d) if div else None
    host = np.full((m * d, ld), sentinel, dtype=T)
    with DeviceBuffers() as dev:
        out = dev.put(host)
        _lib.check(dev.lib.gpx_d_rff_features_grad(_DTYPE_ID[dtype], dev.put(pts), m, d, dev.put(omega), F, scale,
                                                   _lib.dptr(w) if div else None, out, ld, None))
        got = dev.get(out, host)
    p64 = pts.astype(np.float64)
    ref = features_grad_ref(p64, omega, scale, w).reshape(m * d, 2 * F)
    arg = np.abs(p64) @ np.abs(omega).T                                       # sum_k |omega_fk p_ik|: (m, F)
    slope = np.abs(omega.T / (w[:, None] if div else 1.0))                    # |omega_fk / div_k|: (d, F)
    half = (((d + 2) * U * scale * arg + 4 * U * scale)[:, None, :] * slope[None]).reshape(m * d, F)
    bound = np.hstack([half, half])
    if dtype == "float32":
        bound = bound + 2.0 ** -24 * np.abs(ref)
    err = np.abs(got[:, :2 * F].astype(np.float64) - ref)
    print("features' derivative %s (%d, %d, %d) %s: worst err / bound %.3f"
          % (dtype, m, d, F, "col_div" if div else "plain", float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound)
    assert np.all(got[:, 2 * F:] == T(sentinel))                              # the padding keeps its sentinel


# ---- 2. the gradient of K(xo, x) applied to several weight vectors ----
_KGRAD_CASES = [
    # n, m, S, d: the smallest shapes that reach every tail -- n against the 256-point chunk and several slices, m against the
    # points of a workgroup, S against each register block (1, 2, 4 vectors) and more than one group, d against the window
    # (4, 8 or 16 dimensions) and more than one window
    (1, 1, 1, 1), (300, 7, 1, 1), (700, 5, 9, 3), (513, 3, 5, 5), (1000, 2, 33, 17), (2049, 130, 9, 3),
    (300, 7, 2, 3), (300, 3, 2, 17), (300, 3, 1, 17),
]


def _params(d):
    """(h, w): every pair contributes at d > 4."""
    return np.array([1.3, 0.9] if d <= 4 else [3.0, 3.0 * np.sqrt(d)])


def _setup(dev, n, m, S, d, dtype, k_by_apply=False):
    """Points, weights and the pieces of the reference: K from gpx_d_kmat in `dtype`, the differences formed in `dtype`.
    k_by_apply: beyond gpx_d_kmat's own range of d (fp32 d = 95: its tile of column points does not fit) the same elements
    come from the fused gpx_d_kmat_apply on the rows of the identity -- each sum has ONE non-zero term, the element gpx_d_kmat
    would store, and its rounding to `dtype` is exact."""
    T, rng = _NP[dtype], np.random.RandomState(n + m + S + d)
    prm = _params(d)
    x, xo, V = rng.uniform(-3, 3, (n, d)).astype(T), rng.uniform(-3, 3, (m, d)).astype(T), rng.randn(S, n).astype(T)
    dx, dxo, ldk = dev.put(x), dev.put(xo), (n + 15) // 16 * 16
    if k_by_apply:
        Kt = np.zeros((n, m), dtype=T)
        dKt = dev.put(Kt)
        _lib.kapply_fused_max(1 << 20)
        _lib.route_reset()
        rc = dev.lib.gpx_d_kmat_apply(_DTYPE_ID[dtype], _lib.KERNEL_GAUSSIAN, dxo, m, dx, n, d, _lib.dptr(prm), dev.put(np.eye(n, dtype=T)), n,
                                      n, dKt, m, None)
        _lib.kapply_fused_max(-1)
        _lib.check(rc)
        assert _lib.route_count(_lib.ROUTE_KAPPLY_FUSED) == 1 and _lib.route_count(_lib.ROUTE_KAPPLY_GEMM) == 0
        K = dev.get(dKt, Kt).T.astype(np.float64)
    else:
        Kh = np.zeros((m, ldk), dtype=T)
        dK = dev.put(Kh)
        _lib.check(dev.lib.gpx_d_kmat(_DTYPE_ID[dtype], _lib.KERNEL_GAUSSIAN, _lib.K, dxo, m, dx, n, d, _lib.dptr(prm), 0.0, _lib.FULL,
                                      dK, ldk, None))
        K = dev.get(dK, Kh)[:, :n].astype(np.float64)
    diff = (xo[:, None, :] - x[None, :, :]).astype(np.float64)               # formed in T, as the device forms them
    return prm, x, xo, V, dx, dxo, K, diff


def _reference(prm, V, K, diff, div=None):
    """(ref, mag), each (S, m d): -1 / w^2 sum_j V_sj K_ij diff_ijk / div_k and the sum of the terms' magnitudes."""
    S, (m, n, d) = V.shape[0], diff.shape
    terms = (K[:, :, None] * diff) / (prm[1] * prm[1]) / (np.ones(d) if div is None else div)   # (m, n, d)
    V64 = V.astype(np.float64)
    ref = -np.einsum("sj,ijk->sik", V64, terms).reshape(S, m * d)
    mag = np.einsum("sj,ijk->sik", np.abs(V64), np.abs(terms)).reshape(S, m * d)
    return ref, mag


def _kgrad(dev, dtype, dxo, m, dx, n, d, prm, div, dV, ldv, S, dout, ldo, kid=_lib.KERNEL_GAUSSIAN):
    return dev.lib.gpx_d_kmat_apply_grad(_DTYPE_ID[dtype], kid, dxo, m, dx, n, d, _lib.dptr(prm), None if div is None else _lib.dptr(div),
                                         dV, ldv, S, dout, ldo, None)


def _bound(n, eps, mag, total):
    return (n + 4) * U * mag + eps * np.abs(total)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m,S,d", _KGRAD_CASES)
def test_kmat_apply_grad_matches_numpy(n, m, S, d, dtype):
    T, eps = _NP[dtype], _eps(dtype)
    with DeviceBuffers() as dev:
        prm, x, xo, V, dx, dxo, K, diff = _setup(dev, n, m, S, d, dtype)
        out0 = np.random.RandomState(7).randn(S, m * d).astype(T)            # non-zero: the result is accumulated INTO out
        dV = dev.put(V)
        a_buf, b_buf = dev.put(out0), dev.put(out0)
        _lib.check(_kgrad(dev, dtype, dxo, m, dx, n, d, prm, None, dV, n, S, a_buf, m * d))
        _lib.check(_kgrad(dev, dtype, dxo, m, dx, n, d, prm, None, dV, n, S, b_buf, m * d))
        a, b = dev.get(a_buf, out0), dev.get(b_buf, out0)
    ref, mag = _reference(prm, V, K, diff)
    total = ref + out0.astype(np.float64)
    err, bound = np.abs(a.astype(np.float64) - total), _bound(n, eps, mag, total)
    print("kmat_apply_grad %s n=%d m=%d S=%d d=%d: max|ref| %.3e worst err / bound %.3f"
          % (dtype, n, m, S, d, float(np.abs(ref).max()), float((err / np.maximum(bound, 1e-300)).max())))
    if d > 4:
        assert float(np.abs(ref).max()) > 1e-4                               # every pair contributes
    assert np.all(err <= bound)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))                 # two identical calls: identical bits


@pytest.mark.parametrize("dtype,d", [("float64", 47), ("float32", 95)])
def test_kmat_apply_grad_at_the_lds_limit(dtype, d):
    """The largest d whose chunk of x fits 96 KiB of LDS (gpx_d_mean's range), test points included; one more is refused."""
    T, eps, n, m, S = _NP[dtype], _eps(dtype), 300, 5, 4
    with DeviceBuffers() as dev:
        prm, x, xo, V, dx, dxo, K, diff = _setup(dev, n, m, S, d, dtype, k_by_apply=dtype == "float32")
        out0 = np.random.RandomState(7).randn(S, m * d).astype(T)
        buf, dV = dev.put(out0), dev.put(V)
        _lib.check(_kgrad(dev, dtype, dxo, m, dx, n, d, prm, None, dV, n, S, buf, m * d))
        got = dev.get(buf, out0)
        more = np.zeros((n, d + 1), dtype=T)
        big = dev.put(np.zeros((S, m * (d + 1)), dtype=T))
        rc = _kgrad(dev, dtype, dev.put(more[:m]), m, dev.put(more), n, d + 1, prm, None, dV, n, S, big, m * (d + 1))
        assert rc == _lib.ERR_UNSUPPORTED and "too large" in _lib.last_error()
    ref, mag = _reference(prm, V, K, diff)
    total = ref + out0.astype(np.float64)
    assert float(np.abs(ref).max()) > 1e-4
    assert np.all(np.abs(got.astype(np.float64) - total) <= _bound(n, eps, mag, total))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_kmat_apply_grad_takes_any_pitch_and_divides_columns(dtype):
    """V with pitch n + 3 and out with pitch m d + 5, each beginning one element into its block (no 16-byte alignment), and
    column divisors; what lies between the rows keeps its sentinel."""
    T, eps, n, m, S, d, sentinel = _NP[dtype], _eps(dtype), 301, 9, 9, 3, -7.25
    ldv, ldo = n + 3, m * d + 5
    div = np.array([0.7, 1.1, 1.6])
    with DeviceBuffers() as dev:
        prm, x, xo, V, dx, dxo, K, diff = _setup(dev, n, m, S, d, dtype)
        Vraw = np.full(1 + S * ldv, sentinel, dtype=T)
        Vraw[1:].reshape(S, ldv)[:, :n] = V
        oraw = np.full(1 + S * ldo, sentinel, dtype=T)
        out0 = np.random.RandomState(7).randn(S, m * d).astype(T)
        oraw[1:].reshape(S, ldo)[:, :m * d] = out0
        dVraw, doraw = dev.put(Vraw), dev.put(oraw)
        dV, dout = ctypes.c_void_p(dVraw.value + Vraw.itemsize), ctypes.c_void_p(doraw.value + oraw.itemsize)
        _lib.check(_kgrad(dev, dtype, dxo, m, dx, n, d, prm, div, dV, ldv, S, dout, ldo))
        got = dev.get(doraw, oraw)
    ref, mag = _reference(prm, V, K, diff, div)
    total = ref + out0.astype(np.float64)
    block = got[1:].reshape(S, ldo)
    assert np.all(np.abs(block[:, :m * d].astype(np.float64) - total) <= _bound(n, eps, mag, total))
    assert got[0] == T(sentinel) and np.all(block[:, m * d:] == T(sentinel))


def test_kmat_apply_grad_refusals_and_empty_shapes():
    n, m, S, d = 20, 3, 2, 2
    with DeviceBuffers() as dev:
        prm, x, xo, V, dx, dxo, K, diff = _setup(dev, n, m, S, d, "float64")
        out0 = np.random.RandomState(7).randn(S, m * d)
        buf, dV = dev.put(out0), dev.put(V)
        for kid, p in ((_lib.KERNEL_PERIODIC, np.array([1.3, 0.8, 3.0])), (_lib.KERNEL_GAUSSIAN_ARD, np.array([1.3, 0.8, 0.9]))):
            assert _kgrad(dev, "float64", dxo, m, dx, n, d, p, None, dV, n, S, buf, m * d, kid=kid) == _lib.ERR_UNSUPPORTED
            assert "not supported" in _lib.last_error()
        for mm, nn, SS in ((0, n, S), (m, 0, S), (m, n, 0)):                  # nothing to add: out stays as it is
            _lib.check(_kgrad(dev, "float64", dxo, mm, dx, nn, d, prm, None, dV, n, SS, buf, m * d))
        assert np.array_equal(dev.get(buf, out0), out0)
        assert _kgrad(dev, "float64", dxo, m, dx, n, d, prm, None, dV, n - 1, S, buf, m * d) == _lib.ERR_ARG
        assert _kgrad(dev, "float64", dxo, m, dx, n, d, prm, None, dV, n, S, buf, m * d - 1) == _lib.ERR_ARG
        # vector groups (of 4 here) go on the grid's z: more than 65535 of them are refused before anything is launched
        many = 4 * 65535 + 1
        one, wide = dev.put(np.zeros((1, 1))), dev.put(np.zeros((many, 1)))
        assert _kgrad(dev, "float64", one, 1, one, 1, 1, prm, None, wide, 1, many, wide, 1) == _lib.ERR_ARG
        assert "groups of weight vectors" in _lib.last_error()


def test_kmat_apply_grad_at_several_large_d_in_one_process():
    """The chunk of x needs more than 48 KiB of dynamic LDS from d = 24 (fp64) on, and the size follows d: a larger d after a
    smaller one in the same process must still launch.  One register block each: S = 1, 2, 9."""
    dtype, n, m = "float64", 300, 9
    with DeviceBuffers() as dev:
        for d in (26, 40, 26):
            for S in (1, 2, 9):
                prm, x, xo, V, dx, dxo, K, diff = _setup(dev, n, m, S, d, dtype)
                out0 = np.zeros((S, m * d))
                buf = dev.put(out0)
                _lib.check(_kgrad(dev, dtype, dxo, m, dx, n, d, prm, None, dev.put(V), n, S, buf, m * d))
                ref, mag = _reference(prm, V, K, diff)
                assert np.all(np.abs(dev.get(buf, out0) - ref) <= _bound(n, _eps(dtype), mag, ref)), (d, S)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m,d", [(700, 5, 3), (513, 3, 17)])
def test_kmat_apply_grad_of_one_vector_agrees_with_pred_grad(n, m, d, dtype):
    """S = 1 with V = alpha is the gradient of the mean: gpx_d_pred_grad's result, within the same bound (the two kernels'
    sums are ordered differently, so not bitwise)."""
    T, eps = _NP[dtype], _eps(dtype)
    with DeviceBuffers() as dev:
        prm, x, xo, V, dx, dxo, K, diff = _setup(dev, n, m, 1, d, dtype)
        zero, zero64 = np.zeros((1, m * d), dtype=T), np.zeros((m, d))
        buf, pg, dV = dev.put(zero), dev.put(zero64), dev.put(V)
        _lib.check(_kgrad(dev, dtype, dxo, m, dx, n, d, prm, None, dV, n, 1, buf, m * d))
        _lib.check(dev.lib.gpx_d_pred_grad(_DTYPE_ID[dtype], _lib.KERNEL_GAUSSIAN, dxo, m, dx, n, d, _lib.dptr(prm), dV, None, 0, 1.0,
                                           pg, None))
        got, other = dev.get(buf, zero).astype(np.float64).ravel(), dev.get(pg, zero64).ravel()
    ref, mag = _reference(prm, V, K, diff)
    bound = _bound(n, eps, mag, ref).ravel()
    print("one vector against pred_grad %s n=%d d=%d: worst diff / bound %.3f" % (dtype, n, d, float((np.abs(got - other) / bound).max())))
    assert np.all(np.abs(got - other) <= bound)


# ---- 3. paths.grad against the restatement ----
_GREFS = {}


def _gref(kind, dtype, s, S, F, seed, m=300):
    """The restated gradient for a case, computed once and never modified."""
    key = (kind, dtype, s, S, F, seed, m)
    if key not in _GREFS:
        _GREFS[key] = grad_ref(_gp(kind, dtype, s), S, F, seed, _xo(kind, m), dtype=dtype)
    return _GREFS[key]


def _gbound(info, dtype):
    """The project's conditioning bound (cond_bound's form) on the gradient's scale."""
    return C_COND * info["cond"] * _eps(dtype) * info["scale_g"]


def _primitive_bound(info, V, G, n, dtype):
    """(n + 4) u mag + eps |G| of gpx_d_kmat_apply_grad, as (S, m, d), from the restatement's pieces."""
    mag = np.einsum("sj,ijk->sik", np.abs(V), np.abs(info["dK"]))
    return (n + 4) * U * mag + _eps(dtype) * np.abs(G)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("S,F", [(1, 5), (1, 130), (9, 5), (9, 130)])
@pytest.mark.parametrize("kind", ["gauss1", "gauss3", "ard3"])
def test_grad_matches_the_restatement(kind, S, F, dtype):
    s, seed, eps = 0.5, 1000 * S + F, _eps(dtype)
    g, xo = _gp(kind, dtype, s), _xo(kind)
    fr, Gr, info = _gref(kind, dtype, s, S, F, seed)
    paths = g.sample_paths(S, seed=seed, features=F)
    _lib.route_reset()
    one = paths.grad(xo)
    assert _lib.route_count(_lib.ROUTE_PATHS_GRAD_CHUNK) == 1
    _lib.route_reset()
    three = paths.grad(xo, chunk_rows=128)
    assert _lib.route_count(_lib.ROUTE_PATHS_GRAD_CHUNK) == 3
    assert one.shape == (S,) + xo.shape and one.dtype == np.float64 and three.shape == one.shape
    one, three = one.reshape(Gr.shape), three.reshape(Gr.shape)
    err, bound = float(np.abs(one - Gr).max()), _gbound(info, dtype)
    print("grad %s %s S=%d F=%d: err %.3e bound %.3e ratio %.3e" % (kind, dtype, S, F, err, bound, err / bound))
    assert err <= bound and float(np.abs(three - Gr).max()) <= bound
    # the two chunkings: the slice partition depends on m, so not bitwise -- twice the primitive's bound, plus the rounding of
    # the prior term's product of 2F terms
    Vr = paths.state()[2]
    prior = np.einsum("sq,ikq->sik", np.abs(info["theta"]), np.abs(info["psi"]))
    assert np.all(np.abs(one - three) <= 2 * _primitive_bound(info, Vr, Gr, g.x.shape[0], dtype) + 2 * (2 * F + 2) * eps * prior)
    paths.close()
    for call in (paths.grad, paths.value_and_grad):
        with pytest.raises(ValueError, match="closed"):
            call(xo)


# ---- 4. values and gradient from one call ----
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind", ["gauss1", "ard3"])
def test_value_and_grad_is_call_and_grad(kind, dtype):
    g, xo = _gp(kind, dtype, 0.5), _xo(kind)
    paths = g.sample_paths(9, seed=31, features=130)
    for chunk_rows in (0, 128):
        values, grad = paths.value_and_grad(xo, chunk_rows=chunk_rows)
        assert values.shape == (9, 300) and grad.shape == (9,) + xo.shape
        assert np.array_equal(values, paths(xo, chunk_rows=chunk_rows))
        assert np.array_equal(grad, paths.grad(xo, chunk_rows=chunk_rows))
    # values = NULL through the C entry
    pts = np.ascontiguousarray(xo.reshape(300, -1))
    out = np.zeros((9, 300, pts.shape[1]))
    _lib.check(_lib.load().gpx_paths_grad(paths._handle, _lib.dptr(pts), 300, 0, None, _lib.dptr(out)))
    assert np.array_equal(out.reshape(grad.shape), paths.grad(xo))


# ---- 5. the device against central differences of its own values ----
def test_grad_matches_central_differences_of_the_devices_paths():
    """fp64, step 1e-5, tolerance 1e-7 max(1, max|G|) (tests/test_paths_grad_cpu.py's): the sign and the scale, end to end."""
    g, xo, step = _gp("gauss3", "float64", 0.5), _xo("gauss3", 64), 1e-5
    paths = g.sample_paths(5, seed=99, features=64)
    G = paths.grad(xo)
    num = np.empty_like(G)
    for k in range(3):
        e = np.zeros(3)
        e[k] = step
        num[:, :, k] = (paths(xo + e) - paths(xo - e)) / (2 * step)
    err, tol = float(np.abs(G - num).max()), 1e-7 * max(1.0, float(np.abs(G).max()))
    print("central differences: max|G| %.3f err %.3e tol %.3e ratio %.3e" % (float(np.abs(G).max()), err, tol, err / tol))
    assert err <= tol


# ---- 6. housekeeping ----
def test_grad_empty_shapes_and_bad_chunk():
    g = _gp("gauss3", "float64", 0.5)
    xo = _xo("gauss3", 7)
    paths = g.sample_paths(4, seed=5, features=8)
    assert paths.grad(xo[:0]).shape == (4, 0, 3)
    values, grad = paths.value_and_grad(xo[:0])
    assert values.shape == (4, 0) and grad.shape == (4, 0, 3)
    none = g.sample_paths(0, seed=5, features=8)
    assert none.grad(xo).shape == (0, 7, 3) and none.grad(xo[:0]).shape == (0, 0, 3)
    assert [a.shape for a in none.value_and_grad(xo)] == [(0, 7), (0, 7, 3)]
    one = _gp("gauss1", "float64", 0.5).sample_paths(2, seed=5, features=8)
    assert one.grad(np.zeros(0)).shape == (2, 0)
    with pytest.raises(ValueError, match="chunk_rows"):
        paths.grad(xo, chunk_rows=64)
    lib, out = _lib.load(), np.zeros((4, 7, 3))
    assert lib.gpx_paths_grad(paths._handle, _lib.dptr(xo), 7, 64, None, _lib.dptr(out)) == _lib.ERR_ARG
    assert "chunk_rows must be 0 (automatic) or a multiple of 128" in _lib.last_error()


def test_repeated_gradients_reuse_the_handles_buffers():
    """m grows and shrinks between calls on one paths object, values and gradients alternate (its chunk buffers only ever
    grow): the same points give the same bits whatever came before, in both dtypes; so does a fresh object."""
    for dtype in ("float64", "float32"):
        g, xo = _gp("gauss3", dtype, 0.5), _xo("gauss3")
        paths = g.sample_paths(5, seed=77, features=16)
        first = paths.grad(xo[:7])
        values = paths(xo)
        big = paths.grad(xo)
        assert np.array_equal(paths.grad(xo[:7]), first) and np.array_equal(paths.grad(xo), big)
        v, gr = paths.value_and_grad(xo)
        assert np.array_equal(v, values) and np.array_equal(gr, big) and np.array_equal(paths(xo), values)
        fresh = g.sample_paths(5, seed=77, features=16)
        assert np.array_equal(fresh.grad(xo), big)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_grad_prefix_property(dtype):
    """sample_paths(3, seed).grad is the first three of sample_paths(9, seed).grad within the primitive's bound (the groups of
    weight vectors, and with them the slices, differ)."""
    kind, s, F, seed = "gauss3", 0.5, 130, 4242
    g, xo = _gp(kind, dtype, s), _xo(kind)
    small, big = g.sample_paths(3, seed=seed, features=F), g.sample_paths(9, seed=seed, features=F)
    g3, g9 = small.grad(xo), big.grad(xo)
    fr, Gr, info = _gref(kind, dtype, s, 9, F, seed)
    bound = _primitive_bound(info, big.state()[2], Gr, g.x.shape[0], dtype)[:3]
    diff = np.abs(g3 - g9[:3])
    print("prefix %s: worst diff / bound %.3e" % (dtype, float((diff / bound).max())))
    assert np.all(diff <= bound)
    assert float(np.abs(g9 - Gr).max()) <= _gbound(info, dtype)


def test_gradients_outlive_their_gp():
    x, y = _data("d3", 300)
    g = gp.GP(_kernel("gauss3"), x, y, s=0.5)
    xo = _xo("gauss3", 77)
    paths = g.sample_paths(5, seed=31, features=16)
    before = paths.grad(xo)
    g.s = 2.0                                                                # a refit of the source
    g.mean(xo)
    assert np.array_equal(paths.grad(xo), before)
    del g
    gc.collect()
    assert np.array_equal(paths.grad(xo), before)
    again = gp.GP(_kernel("gauss3"), x, y, s=0.5).sample_paths(5, seed=31, features=16)
    assert np.array_equal(again.grad(xo), before)                            # a pure function of (seed, size, features) and the fit


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_grad_ard_at_equal_widths_agrees_with_gaussian(dtype):
    S, F, seed, s = 9, 130, 77, 0.5
    xo = _xo("gauss3")
    iso, ard = _gp("gauss3", dtype, s), _gp("ard3_equal", dtype, s)
    a, b = iso.sample_paths(S, seed=seed, features=F).grad(xo), ard.sample_paths(S, seed=seed, features=F).grad(xo)
    bound = _gbound(_gref("gauss3", dtype, s, S, F, seed)[2], dtype) + _gbound(_gref("ard3_equal", dtype, s, S, F, seed)[2], dtype)
    err = float(np.abs(a - b).max())
    print("ARD at equal widths %s: err %.3e bound %.3e ratio %.3e" % (dtype, err, bound, err / bound))
    assert err <= bound
