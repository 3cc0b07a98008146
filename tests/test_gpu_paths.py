"""GPU tests of GP.sample_paths: the two device primitives (gpx_d_rff_features, gpx_d_kmat_apply on both of its routes), the
state of a paths handle against the numpy restatement of its definition (tests/_paths_helpers.py), PosteriorPaths.__call__,
and the semantics (prefix property, independence of the source GP, ARD at equal widths).

Bounds.  u = 2^-53, eps = the dtype's machine epsilon.
  features  fp64: (d + 2) u sum_k |omega_fk p_ik| scale + 4 u scale -- the rounding of the projection on both sides carried
            through cos / sin (slope <= 1), plus a few ulp of sincos and of the product with scale; fp32: + 2^-24 |ref|, the store.
  kmat_apply against K V^T in float64 with K from gpx_d_kmat in the same dtype (the same entry function):
            fused, and the product route in fp64: (n + 2) u sum_j |K_ij V_sj| + eps |ref| (f64 sums, one rounding to dtype);
            product route in fp32: n eps sum_j |K_ij V_sj| (an fp32 MFMA product).  These are measured into a ZERO block; a
            preloaded block is then compared with preload + that result within eps (|preload| + |result|): one more addition.
  state     Omega, Theta: the tolerances of tests/test_gpu_sample.py::test_randn_matches_the_restatement (Omega = z / w_v: / w_v).
            V, free of the condition number: Cholesky solves are backward stable, |Kxx x - b| <= c n eps |Kxx| |x| normwise, for
            alpha and for R = Kxx^-1 r alike; the device's r differs from the restatement's by the rounding of the features, of a
            product of 2F terms and of sigma E:
              |Kxx V_s - (y - r_s)| <= eps [4 n |Kxx|_inf (|alpha|_inf + |Kxx^-1 r_s|_inf + |V_s|_inf)
                                            + (2F + 4) (max_j sum_q |Phi_jq Theta_sq| + sigma max_j |E_sj|) + max |y|]
            V and f against the restatement: the project's C_COND cond(Kxx) eps scale (tests/_paths_helpers.py: cond_bound)."""
import ctypes
import gc

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from conftest import load_golden
from _extend_helpers import DeviceBuffers
from _paths_helpers import cond_bound, features_ref, paths_ref, stored
from _sample_helpers import randn_ref

pytestmark = pytest.mark.gpu

_DTYPE_ID = {"float64": _lib.F64, "float32": _lib.F32}
_NP = {"float64": np.float64, "float32": np.float32}
U = 2.0 ** -53


def _eps(dtype):
    return float(np.finfo(_NP[dtype]).eps)


@pytest.fixture
def routes():
    """Force a route of gpx_d_kmat_apply through GPX_KAPPLY_FUSED_MAX; the default is restored afterwards."""
    def force(route):
        _lib.kapply_fused_max(1 << 20 if route == "fused" else 0)
        _lib.route_reset()
    yield force
    _lib.kapply_fused_max(-1)


def _took(route):
    fused, gemm = _lib.route_count(_lib.ROUTE_KAPPLY_FUSED), _lib.route_count(_lib.ROUTE_KAPPLY_GEMM)
    return (fused > 0 and gemm == 0) if route == "fused" else (gemm > 0 and fused == 0)


# ---- 1. the feature map ----
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("m,d,F,ld", [(1, 1, 1, 16), (7, 3, 5, 16), (300, 3, 130, 272), (257, 7, 64, 128)])
def test_rff_features_match_the_restatement(m, d, F, ld, dtype):
    T, rng, scale, sentinel = _NP[dtype], np.random.RandomState(m + F), 0.37, -7.25
    pts = rng.uniform(-10, 10, (m, d)).astype(T)
    omega = rng.randn(F, d) / 0.7
    host = np.full((m, ld), sentinel, dtype=T)
    with DeviceBuffers() as dev:
        out = dev.put(host)
        _lib.check(dev.lib.gpx_d_rff_features(_DTYPE_ID[dtype], dev.put(pts), m, d, dev.put(omega), F, scale, out, ld, None))
        got = dev.get(out, host)
    p64 = pts.astype(np.float64)
    ref = features_ref(p64, omega, scale)
    arg = np.abs(p64) @ np.abs(omega).T                                       # sum_k |omega_fk p_ik|
    bound = np.hstack([arg, arg]) * (d + 2) * U * scale + 4 * U * scale
    if dtype == "float32":
        bound = bound + 2.0 ** -24 * np.abs(ref)
    err = np.abs(got[:, :2 * F].astype(np.float64) - ref)
    print("features %s (%d, %d, %d): worst err / bound %.3f" % (dtype, m, d, F, float((err / bound).max())))
    assert np.all(err <= bound)
    assert np.all(got[:, 2 * F:] == T(sentinel))                              # the padding keeps its sentinel


# ---- 2. K(xo, x) applied to several weight vectors, both routes ----
_KAPPLY_CASES = [
    # n, m, S, d, kernel: the smallest shapes that reach every tail (n vs the 256-point chunk, m vs 4 points a workgroup, S vs the
    # register block of 8 and more than one block, several slices: n = 700 with few points)
    (1, 1, 1, 1, "gaussian"), (255, 7, 3, 3, "gaussian"), (257, 9, 8, 7, "gaussian"), (700, 7, 9, 3, "gaussian"),
    (700, 300, 20, 3, "gaussian"), (255, 1, 1, 7, "gaussian"), (257, 300, 9, 1, "periodic"), (700, 9, 20, 3, "periodic"),
    # each register block (8 x 1 for S = 1, 8 x 4 for S <= 4, 4 x 8 beyond) with more than one workgroup along m and an m % 8 tail
    (700, 300, 3, 3, "gaussian"), (257, 9, 1, 3, "gaussian"),
]


def _kapply(dev, dtype, kid, dxo, m, dx, n, d, prm, dV, ldv, S, out0, ldo):
    buf = dev.put(out0)
    _lib.check(dev.lib.gpx_d_kmat_apply(_DTYPE_ID[dtype], kid, dxo, m, dx, n, d, _lib.dptr(prm), dV, ldv, S, buf, ldo, None))
    return dev.get(buf, out0)


@pytest.mark.parametrize("route", ["fused", "gemm"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n,m,S,d,kernel", _KAPPLY_CASES)
def test_kmat_apply_both_routes(n, m, S, d, kernel, dtype, route, routes):
    T, eps, rng = _NP[dtype], _eps(dtype), np.random.RandomState(n + m + S)
    kid = _lib.KERNEL_GAUSSIAN if kernel == "gaussian" else _lib.KERNEL_PERIODIC
    prm = np.array([1.3, 0.9] if kernel == "gaussian" else [1.3, 0.8, 3.0])
    x, xo = rng.uniform(-3, 3, (n, d)).astype(T), rng.uniform(-3, 3, (m, d)).astype(T)
    ldv, ldo, ldk, sentinel = (n + 15) // 16 * 16 + 16, m + 5, (n + 15) // 16 * 16, -7.25
    V = np.full((S, ldv), sentinel, dtype=T)
    V[:, :n] = rng.randn(S, n)
    zero = np.full((S, ldo), sentinel, dtype=T)
    zero[:, :m] = 0
    pre = zero.copy()
    pre[:, :m] = rng.randn(S, m)
    with DeviceBuffers() as dev:
        dx, dxo, dV = dev.put(x), dev.put(xo), dev.put(V)
        Kh = np.zeros((m, ldk), dtype=T)
        dK = dev.put(Kh)
        _lib.check(dev.lib.gpx_d_kmat(_DTYPE_ID[dtype], kid, _lib.K, dxo, m, dx, n, d, _lib.dptr(prm), 0.0, _lib.FULL, dK, ldk, None))
        K = dev.get(dK, Kh)[:, :n].astype(np.float64)
        routes(route)
        a = _kapply(dev, dtype, kid, dxo, m, dx, n, d, prm, dV, ldv, S, zero, ldo)
        assert _took(route)
        b = _kapply(dev, dtype, kid, dxo, m, dx, n, d, prm, dV, ldv, S, zero, ldo)
        c = _kapply(dev, dtype, kid, dxo, m, dx, n, d, prm, dV, ldv, S, pre, ldo)
    V64 = V[:, :n].astype(np.float64)
    ref, mag = V64 @ K.T, np.abs(V64) @ np.abs(K).T
    if route == "gemm" and dtype == "float32":
        bound = n * eps * mag
    else:
        bound = (n + 2) * U * mag + eps * np.abs(ref)
    got = a[:, :m].astype(np.float64)
    err = np.abs(got - ref)
    print("kmat_apply %s %s %s n=%d m=%d S=%d d=%d: worst err / bound %.3f"
          % (route, dtype, kernel, n, m, S, d, float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))                 # two identical calls: identical bits
    p64 = pre[:, :m].astype(np.float64)
    assert np.all(np.abs(c[:, :m].astype(np.float64) - (p64 + got)) <= eps * (np.abs(p64) + np.abs(got)))   # accumulated, not overwritten
    for r in (a, c):
        assert np.all(r[:, m:] == T(sentinel))


def test_kmat_apply_beyond_the_fused_range_takes_the_product(routes):
    """d = 64 in fp64 needs more than 96 KiB of LDS for a chunk of x (gpx_d_mean's limit; gpx_d_kmat still takes it): the call
    takes the product route whatever the switch says."""
    n, m, S, d = 64, 5, 2, 64
    rng = np.random.RandomState(3)
    x, xo, V = rng.uniform(-1, 1, (n, d)), rng.uniform(-1, 1, (m, d)), rng.randn(S, n)
    prm = np.array([1.3, 9.0])
    with DeviceBuffers() as dev:
        routes("fused")
        got = _kapply(dev, "float64", _lib.KERNEL_GAUSSIAN, dev.put(xo), m, dev.put(x), n, d, prm, dev.put(V), n, S, np.zeros((S, m)), m)
    assert _took("gemm")
    K = gp.GaussianKernel(1.3, 9.0)(xo, x)
    np.testing.assert_allclose(got, V @ K.T, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("dtype,ds", [("float64", (26, 40, 26)), ("float32", (64, 90, 50))])
def test_kmat_apply_fused_at_several_large_d_in_one_process(dtype, ds, routes):
    """The chunk of x needs more than 48 KiB of dynamic LDS from d = 24 (fp64) / 48 (fp32) on, and the size follows d: a
    larger d after a smaller one in the same process must still launch (the kernel's limit is set for the largest chunk,
    not for the first call's).  One register block each: S = 1, 3, 9.  Reference and bound as above."""
    T, eps, n, m = _NP[dtype], _eps(dtype), 300, 9
    with DeviceBuffers() as dev:
        for d in ds:
            for S in (1, 3, 9):
                rng = np.random.RandomState(d + S)
                prm = np.array([1.3, 0.5 * np.sqrt(d)])
                x, xo, V = rng.uniform(-1, 1, (n, d)).astype(T), rng.uniform(-1, 1, (m, d)).astype(T), rng.randn(S, n).astype(T)
                dx, dxo, ldk = dev.put(x), dev.put(xo), 304
                Kh = np.zeros((m, ldk), dtype=T)
                dK = dev.put(Kh)
                _lib.check(dev.lib.gpx_d_kmat(_DTYPE_ID[dtype], _lib.KERNEL_GAUSSIAN, _lib.K, dxo, m, dx, n, d, _lib.dptr(prm), 0.0,
                                              _lib.FULL, dK, ldk, None))
                K = dev.get(dK, Kh)[:, :n].astype(np.float64)
                routes("fused")
                got = _kapply(dev, dtype, _lib.KERNEL_GAUSSIAN, dxo, m, dx, n, d, prm, dev.put(V), n, S, np.zeros((S, m), dtype=T), m)
                assert _took("fused")
                V64 = V.astype(np.float64)
                ref, mag = V64 @ K.T, np.abs(V64) @ np.abs(K).T
                assert np.all(np.abs(got.astype(np.float64) - ref) <= (n + 2) * U * mag + eps * np.abs(ref)), (d, S)


@pytest.mark.parametrize("route", ["fused", "gemm"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_kmat_apply_takes_any_pitch_of_V(dtype, route, routes):
    """ldv = n + 3 and a base that is not 16-byte aligned: both routes accept what the other accepts."""
    T, eps, n, m, S, d = _NP[dtype], _eps(dtype), 301, 9, 9, 3
    rng = np.random.RandomState(5)
    prm, ldv = np.array([1.3, 0.9]), n + 3
    x, xo = rng.uniform(-3, 3, (n, d)).astype(T), rng.uniform(-3, 3, (m, d)).astype(T)
    V = rng.randn(1 + S * ldv).astype(T)                                     # the matrix begins at element 1
    with DeviceBuffers() as dev:
        dx, dxo, dVraw = dev.put(x), dev.put(xo), dev.put(V)
        dV = ctypes.c_void_p(dVraw.value + V.itemsize)
        Kh = np.zeros((m, 304), dtype=T)
        dK = dev.put(Kh)
        _lib.check(dev.lib.gpx_d_kmat(_DTYPE_ID[dtype], _lib.KERNEL_GAUSSIAN, _lib.K, dxo, m, dx, n, d, _lib.dptr(prm), 0.0, _lib.FULL,
                                      dK, 304, None))
        K = dev.get(dK, Kh)[:, :n].astype(np.float64)
        routes(route)
        got = _kapply(dev, dtype, _lib.KERNEL_GAUSSIAN, dxo, m, dx, n, d, prm, dV, ldv, S, np.zeros((S, m), dtype=T), m)
        assert _took(route)
    V64 = V[1:].reshape(S, ldv)[:, :n].astype(np.float64)
    ref, mag = V64 @ K.T, np.abs(V64) @ np.abs(K).T
    bound = n * eps * mag if (route == "gemm" and dtype == "float32") else (n + 2) * U * mag + eps * np.abs(ref)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= bound)


# ---- 3. the state of a paths handle ----
_GPS, _REFS = {}, {}


def _data(kind, n):
    rng = np.random.RandomState(n)
    if kind == "gauss1":
        x = np.linspace(-10, 10, n) + rng.uniform(-0.02, 0.02, n)             # spacing 0.1 against a width of 0.08: s = 0 stays well conditioned
        return x, np.sin(x) + 0.3 * np.cos(3 * x)
    x = rng.uniform(-10, 10, (n, 3))
    return x, np.sin(x[:, 0]) + 0.3 * np.cos(x[:, 1] - 0.5 * x[:, 2])


def _kernel(kind):
    if kind == "gauss1":
        return gp.GaussianKernel(1.2, 0.08)
    if kind == "gauss3":
        return gp.GaussianKernel(1.0, 0.5 * np.sqrt(3))
    if kind == "ard3_equal":
        return gp.GaussianARDKernel(1.0, [0.5 * np.sqrt(3)] * 3)
    return gp.GaussianARDKernel(1.0, [0.7, 1.1, 1.6])


_N = {"gauss1": 200, "gauss3": 700, "ard3": 300, "ard3_equal": 700}


def _gp(kind, dtype, s):
    """One fitted GP per (kind, dtype, s), shared and never modified."""
    key = (kind, dtype, s)
    if key not in _GPS:
        x, y = _data("gauss1" if kind == "gauss1" else "d3", _N[kind])
        _GPS[key] = gp.GP(_kernel(kind), x, y, s=s, dtype=dtype)
    return _GPS[key]


def _xo(kind, m=300):
    pts = np.random.RandomState(11).uniform(-10, 10, (300, 3))[:m]
    return pts[:, 0].copy() if kind == "gauss1" else pts


def _ref(kind, dtype, s, S, F, seed, m=300):
    """The restatement for a case, computed once."""
    key = (kind, dtype, s, S, F, seed, m)
    if key not in _REFS:
        _REFS[key] = paths_ref(_gp(kind, dtype, s), S, F, seed, xo=_xo(kind, m), dtype=dtype)
    return _REFS[key]


_STATE_CASES = [("gauss1", 1, 5, 0.5), ("gauss1", 9, 130, 0.0), ("gauss3", 9, 130, 0.5), ("gauss3", 1, 5, 0.0),
                ("ard3", 9, 5, 0.5), ("ard3", 1, 130, 0.0)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind,S,F,s", _STATE_CASES)
def test_state_matches_the_restatement(kind, S, F, s, dtype):
    g, seed, eps = _gp(kind, dtype, s), 1000 * S + F, _eps(dtype)
    paths = g.sample_paths(S, seed=seed, features=F)
    assert (paths.size, paths.features, paths.seed, paths.n, paths.d) == (S, F, seed, g.x.shape[0], 1 if kind == "gauss1" else 3)
    omega, theta, V = paths.state()
    Vr, _, info = _ref(kind, dtype, s, S, F, seed)
    w_v = info["view"][2]
    assert float(np.abs(omega - info["omega"]).max()) <= 1e-13 / w_v
    tr = randn_ref(S, 2 * F, seed, stream=2)
    if dtype == "float64":
        assert float(np.abs(theta - tr).max()) <= 1e-13
    else:
        assert np.all(np.abs(theta - stored(tr, dtype)) <= 2.0 ** -23 * np.maximum(np.abs(tr), 1.0))
    # free of the condition number: the residual of Kxx V_s = y - r_s, Kxx as the device built it
    Kxx, n = g.Kxx, g.x.shape[0]
    res = np.abs(V @ Kxx.T - (g.y - info["r"]))
    Kir = info["alpha"] - Vr
    solve = 4 * n * float(np.abs(Kxx).sum(axis=1).max()) * (float(np.abs(info["alpha"]).max()) + np.abs(Kir).max(axis=1) + np.abs(V).max(axis=1))
    made = (2 * F + 4) * ((np.abs(info["theta"]) @ np.abs(info["Phi"]).T).max(axis=1) + s * np.abs(info["E"]).max(axis=1))
    rbound = eps * (solve + made + float(np.abs(g.y).max()))
    print("state %s %s S=%d F=%d s=%g: residual / bound %.3e" % (kind, dtype, S, F, s, float((res.max(axis=1) / rbound).max())))
    assert np.all(res.max(axis=1) <= rbound)
    # against the restatement, within the project's conditioning bound
    err, bound = float(np.abs(V - Vr).max()), cond_bound(info, dtype, "V")
    print("state %s %s S=%d F=%d s=%g: V err %.3e bound %.3e ratio %.3e cond %.3e" % (kind, dtype, S, F, s, err, bound, err / bound, info["cond"]))
    assert err <= bound


# ---- 4. evaluation ----
@pytest.mark.parametrize("route", ["fused", "gemm"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind,S,F,s", [("gauss1", 9, 130, 0.5), ("gauss3", 9, 130, 0.5), ("ard3", 9, 5, 0.5), ("gauss3", 1, 5, 0.0)])
def test_call_matches_the_restatement(kind, S, F, s, dtype, route, routes):
    g, seed, xo, eps = _gp(kind, dtype, s), 1000 * S + F, _xo(kind), _eps(dtype)
    Vr, fr, info = _ref(kind, dtype, s, S, F, seed)
    paths = g.sample_paths(S, seed=seed, features=F)
    routes(route)
    one = paths(xo)
    assert _took(route) and _lib.route_count(_lib.ROUTE_KAPPLY_FUSED) + _lib.route_count(_lib.ROUTE_KAPPLY_GEMM) == 1
    routes(route)
    three = paths(xo, chunk_rows=128)
    assert _took(route) and _lib.route_count(_lib.ROUTE_KAPPLY_FUSED) + _lib.route_count(_lib.ROUTE_KAPPLY_GEMM) == 3
    assert one.shape == (S, 300) and one.dtype == np.float64
    err, bound = float(np.abs(one - fr).max()), cond_bound(info, dtype, "f")
    print("call %s %s %s S=%d F=%d: err %.3e bound %.3e ratio %.3e" % (kind, dtype, route, S, F, err, bound, err / bound))
    assert err <= bound and float(np.abs(three - fr).max()) <= bound
    # the two chunkings: the slice partition depends on m, so not bitwise -- twice the bound of one application, plus the
    # rounding of the prior term's product of 2F terms
    n = g.x.shape[0]
    mag, prior = np.abs(Vr) @ np.abs(info["Ko"]).T, np.abs(info["theta"]) @ np.abs(info["phi_o"]).T
    kb = n * eps * mag if (route == "gemm" and dtype == "float32") else (n + 2) * U * mag + eps * np.abs(fr)
    assert np.all(np.abs(one - three) <= 2 * kb + 2 * (2 * F + 2) * eps * prior)
    paths.close()
    with pytest.raises(ValueError, match="closed"):
        paths(xo)


def test_repeated_evaluations_reuse_the_handles_buffers():
    """m grows and shrinks between calls on one paths object (its chunk buffers only ever grow): the same points give the
    same bits whatever came before, in both dtypes."""
    for dtype in ("float64", "float32"):
        g, xo = _gp("gauss3", dtype, 0.5), _xo("gauss3")
        paths = g.sample_paths(5, seed=77, features=16)
        first = paths(xo[:7])
        big = paths(xo)
        assert np.array_equal(paths(xo[:7]), first) and np.array_equal(paths(xo), big)
        fresh = g.sample_paths(5, seed=77, features=16)
        assert np.array_equal(fresh(xo), big)


def test_empty_shapes():
    g = _gp("gauss3", "float64", 0.5)
    xo = _xo("gauss3", 7)
    paths = g.sample_paths(4, seed=5, features=8)
    assert paths(xo[:0]).shape == (4, 0)
    none = g.sample_paths(0, seed=5, features=8)
    assert none(xo).shape == (0, 7) and none(xo[:0]).shape == (0, 0)
    assert [a.shape for a in none.state()] == [(8, 3), (0, 16), (0, 700)]
    with pytest.raises(ValueError, match="chunk_rows"):
        paths(xo, chunk_rows=64)
    lib, out = _lib.load(), np.zeros((4, 7))
    assert lib.gpx_paths_eval(paths._handle, _lib.dptr(xo), 7, 64, _lib.dptr(out)) == _lib.ERR_ARG
    assert "chunk_rows must be 0 (automatic) or a multiple of 128" in _lib.last_error()
    dt, kid, n, d, S, F, seed = (ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(),
                                 ctypes.c_uint64())
    _lib.check(lib.gpx_paths_describe(paths._handle, *(ctypes.byref(v) for v in (dt, kid, n, d, S, F, seed))))
    assert (dt.value, kid.value, n.value, d.value, S.value, F.value, seed.value) == (_lib.F64, _lib.KERNEL_GAUSSIAN, 700, 3, 4, 8, 5)


# ---- 5. the prefix property ----
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_prefix_property(dtype):
    kind, s, F, seed = "gauss3", 0.5, 130, 4242
    g, xo = _gp(kind, dtype, s), _xo(kind)
    small, big = g.sample_paths(3, seed=seed, features=F), g.sample_paths(9, seed=seed, features=F)
    (o3, t3, v3), (o9, t9, v9) = small.state(), big.state()
    assert np.array_equal(o3, o9) and np.array_equal(t3, t9[:3])
    # the noise rows: row s of stream 3 is the same whatever the number of rows
    n, T = g.x.shape[0], _NP[dtype]
    with DeviceBuffers() as dev:
        h3, h9 = np.zeros((3, n), dtype=T), np.zeros((9, n), dtype=T)
        b3, b9 = dev.put(h3), dev.put(h9)
        for buf, rows in ((b3, 3), (b9, 9)):
            _lib.check(dev.lib.gpx_d_randn(_DTYPE_ID[dtype], buf, rows, n, n, seed, 3, 0, None))
        assert np.array_equal(dev.get(b3, h3), dev.get(b9, h9)[:3])
    _, fr, info = _ref(kind, dtype, s, 9, F, seed)
    assert float(np.abs(v3 - v9[:3]).max()) <= 2 * cond_bound(info, dtype, "V")
    assert float(np.abs(small(xo) - big(xo)[:3]).max()) <= 2 * cond_bound(info, dtype, "f")
    assert float(np.abs(big(xo) - fr).max()) <= cond_bound(info, dtype, "f")


# ---- 6. independence of the source ----
def test_paths_outlive_their_gp():
    x, y = _data("d3", 300)
    g = gp.GP(_kernel("gauss3"), x, y, s=0.5)
    xo = _xo("gauss3", 77)
    g.mean(xo)
    _lib.route_reset()
    paths = g.sample_paths(5, seed=31, features=16)
    before = paths(xo)
    for r in (_lib.ROUTE_SAMPLE, _lib.ROUTE_VAR_CHUNK, _lib.ROUTE_LOO_CHUNK, _lib.ROUTE_GRAD_CHUNK, _lib.ROUTE_EXTEND):
        assert _lib.route_count(r) == 0
    assert _lib.route_count(_lib.ROUTE_KAPPLY_FUSED) == 1
    mean = g.mean(xo)
    g.s = 2.0                                                                # a refit of the source
    assert not np.array_equal(g.mean(xo), mean)
    assert np.array_equal(paths(xo), before)
    del g
    gc.collect()
    assert np.array_equal(paths(xo), before)
    again = gp.GP(_kernel("gauss3"), x, y, s=0.5).sample_paths(5, seed=31, features=16)
    assert np.array_equal(again(xo), before)                                 # a pure function of (seed, size, features) and the fit


def test_paths_not_positive_definite():
    rec = load_golden("gp_nonpd.npz")
    hh, w, s = rec["params"]
    bad = gp.GP(gp.GaussianKernel(hh, w), rec["x"], rec["y"], s=s)
    with pytest.raises(np.linalg.LinAlgError):
        bad.sample_paths(2, seed=1)
    h = ctypes.c_void_p(5)
    rc = _lib.load().gpx_gp_paths_create(bad._fit().handle, 2, 8, 1, ctypes.byref(h))
    assert rc == _lib.ERR_ARG and "not positive definite" in _lib.last_error() and not h
    good = _gp("gauss3", "float64", 0.5)._fit().handle
    assert _lib.load().gpx_gp_paths_create(good, -1, 8, 1, ctypes.byref(h)) == _lib.ERR_ARG
    assert _lib.load().gpx_gp_paths_create(good, 2, 0, 1, ctypes.byref(h)) == _lib.ERR_ARG
    per = gp.GP(gp.PeriodicKernel(1.0, 0.8, 3.0), np.linspace(0, 5, 20), np.zeros(20), s=1.0)
    assert _lib.load().gpx_gp_paths_create(per._fit().handle, 2, 8, 1, ctypes.byref(h)) == _lib.ERR_UNSUPPORTED


# ---- 7. ARD at equal widths is the Gaussian kernel ----
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_ard_at_equal_widths_agrees_with_gaussian(dtype):
    S, F, seed, s = 9, 130, 77, 0.5
    xo = _xo("gauss3")
    iso, ard = _gp("gauss3", dtype, s), _gp("ard3_equal", dtype, s)
    a, b = iso.sample_paths(S, seed=seed, features=F)(xo), ard.sample_paths(S, seed=seed, features=F)(xo)
    bound = cond_bound(_ref("gauss3", dtype, s, S, F, seed)[2], dtype, "f") + cond_bound(_ref("ard3_equal", dtype, s, S, F, seed)[2], dtype, "f")
    err = float(np.abs(a - b).max())
    print("ARD at equal widths %s: err %.3e bound %.3e ratio %.3e" % (dtype, err, bound, err / bound))
    assert err <= bound
