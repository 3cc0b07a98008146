"""GPU tests of GP.sample (gpx_gp_sample, gpx_gp_sample_from_K), of gpx_d_mvn_sample and of the generator gpx_d_randn.

The generator is pinned element by element to its numpy restatement (tests/_sample_helpers.py, itself pinned to the
Random123 known answers in tests/test_sample_cpu.py):
  fp64  |got - ref| <= 1e-13: the angle 2 pi u2 carries at most 1.2e-15 of rounding on the numpy side (the device's
        sincospi(2 u2) none), log, sqrt, sin and cos are good to a few ulp on both sides and r <= 8.6, so an honest
        difference is at most about 1e-14; the bound is ten times that.
  fp32  |got - float32(ref)| <= 2^-23 max(|ref|, 1): one rounding step.
The samples are pinned to their own reconstruction  mean + Z chol(A)^T,  A = cov + (jitter [+ s^2]) I,  from the GP's own
`mean` and `cov` (older code, pinned to the oracle by the existing suites) within the project's bound
C_COND cond(A) eps_dtype scale, C_COND = 16 (tests/test_gpu_parity.py), scale = max|mean| + max_s sum_k |Z_sk| sqrt(max diag A);
and, independently of the device's `cov`, to the oracle within ORACLE_TOL of tests/test_gpu_var.py.  There is no
statistical test here: with the generator pinned element by element and the samples pinned to mean + Z L^T, a moment test
would add a tolerance and no coverage."""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from conftest import load_golden
from test_dist_gp_cpu import _PythonRBF
from _extend_helpers import ARD_W, DeviceBuffers, case, make_kernel
from _sample_helpers import C_COND, randn_ref, reconstruction

pytestmark = pytest.mark.gpu

ORACLE_TOL = {"float64": dict(rtol=1e-7, atol=1e-10), "float32": dict(rtol=1e-2, atol=5e-3)}      # tests/test_gpu_var.py
_DTYPE_ID = {"float64": _lib.F64, "float32": _lib.F32}
_NP = {"float64": np.float64, "float32": np.float32}
M_MAX = 300


def _xo(kind, m=M_MAX):
    """The first m of M_MAX test points in the box of the training inputs (one draw per dimension count)."""
    d = 1 if kind == "periodic" else 3
    pts = np.random.RandomState(11).uniform(-10, 10, (M_MAX, d))[:m]
    return pts.ravel() if d == 1 else pts


def _within(got, ref, bound, what):
    err = float(np.abs(got - ref).max())
    print("%s: err %.3e bound %.3e ratio %.3e" % (what, err, bound, err / bound))
    assert got.shape == ref.shape
    assert err <= bound, "%s: |got - ref| = %.3e exceeds C_COND cond eps scale = %.3e" % (what, err, bound)


# ---- 1. the generator against the restatement ----
def _randn(dev, dtype, rows, cols, ld, seed, stream=0, offset=0, sentinel=-7.25, row0=0, into=None):
    T = _NP[dtype]
    host = np.full((rows, ld), sentinel, dtype=T)
    buf = dev.put(host) if into is None else into
    ptr = ctypes.c_void_p(buf.value + row0 * ld * host.itemsize)
    _lib.check(dev.lib.gpx_d_randn(_DTYPE_ID[dtype], ptr, rows, cols, ld, seed, stream, offset, None))
    return buf, host


def _check_randn(got, ref, dtype):
    if dtype == "float64":
        err = float(np.abs(got - ref).max())
        print("randn fp64: err %.3e" % err)
        assert err <= 1e-13
    else:
        err = np.abs(got.astype(np.float64) - ref.astype(np.float32).astype(np.float64))
        assert np.all(err <= 2.0 ** -23 * np.maximum(np.abs(ref), 1.0)), float(err.max())


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("rows,cols,ld,seed,stream,offset", [
    (1, 1, 16, 5, 0, 0),
    (3, 5, 5, 12345, 0, 0),                               # a pair straddles a row
    (257, 130, 144, 2 ** 64 - 1, 0, 0),                   # more than one workgroup; padding
    (2, 7, 7, 99, 2 ** 32 + 3, 2 ** 33 + 1),              # the high counter words, an odd start
], ids=["1x1", "3x5", "257x130_ld144", "2x7_high_words"])
def test_randn_matches_the_restatement(rows, cols, ld, seed, stream, offset, dtype):
    with DeviceBuffers() as dev:
        buf, host = _randn(dev, dtype, rows, cols, ld, seed, stream, offset)
        got = dev.get(buf, host)
    _check_randn(got[:, :cols], randn_ref(rows, cols, seed, stream, offset), dtype)
    assert np.all(got[:, cols:] == host[:, cols:])                          # the padding still holds the sentinel


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("rows,cols,ld,split", [(5, 7, 16, 2), (257, 130, 144, 100), (4, 3, 3, 1)])
def test_randn_split_by_rows_gives_the_same_bits(rows, cols, ld, split, dtype):
    seed = 31337
    with DeviceBuffers() as dev:
        one, host = _randn(dev, dtype, rows, cols, ld, seed)
        two, _ = _randn(dev, dtype, split, cols, ld, seed, into=dev.put(host))
        _randn(dev, dtype, rows - split, cols, ld, seed, offset=split * cols, row0=split, into=two)
        a, b = dev.get(one, host), dev.get(two, host)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert not np.any(a[:, :cols] == host[:, :cols])


# ---- 2. gpx_d_mvn_sample directly ----
def _mvn(dev, dtype, C, mean, jitter, S, seed):
    T = _NP[dtype]
    m, ldc = C.shape[0], 16
    Cp = np.full((m, ldc), 7.25, dtype=T)
    Cp[:, :m] = np.tril(C) + np.triu(np.full((m, m), 7.25), 1)              # the strict upper triangle is never read
    out0 = np.full((max(S, 1), ldc), -7.25, dtype=T)
    dC, dZ, dout = dev.put(Cp), dev.put(out0), dev.put(out0)
    dmean = dev.put(np.asarray(mean, dtype=T)) if mean is not None else None
    dinfo = dev.put(np.array([-9], dtype=np.int32))
    _lib.check(dev.lib.gpx_d_mvn_sample(_DTYPE_ID[dtype], dC, m, ldc, dmean, jitter, S, seed, 0, dZ, ldc, dout, ldc, dinfo, None))
    return dev.get(dC, Cp), dev.get(dout, out0), int(dev.get(dinfo, np.zeros(1, dtype=np.int32))[0])


def test_mvn_sample_indefinite_leaves_info():
    with DeviceBuffers() as dev:
        _, _, info = _mvn(dev, "float64", np.array([[1.0, 2.0], [2.0, 1.0]]), None, 0.0, 1, 1)
    assert info == 2


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("with_mean", [True, False])
def test_mvn_sample_3x3(with_mean, dtype):
    T, eps = _NP[dtype], float(np.finfo(_NP[dtype]).eps)
    C = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, -0.25], [0.5, -0.25, 2.0]]).astype(T).astype(np.float64)
    mean = np.array([0.5, -1.5, 2.0]) if with_mean else None
    jitter, S, seed = 0.125, 4, 77
    with DeviceBuffers() as dev:
        Lc, out, info = _mvn(dev, dtype, C, mean, jitter, S, seed)
    assert info == 0
    A = C + jitter * np.eye(3)
    L = np.linalg.cholesky(A)
    Z = randn_ref(S, 3, seed)
    m0 = mean if with_mean else np.zeros(3)
    ref = m0 + Z @ L.T
    scale = float(np.abs(m0).max()) + float(np.abs(Z).sum(axis=1).max()) * np.sqrt(float(np.diag(A).max()))
    cond = float(np.linalg.cond(A))
    _within(out[:S, :3].astype(np.float64), ref, C_COND * cond * eps * scale, "mvn_sample 3x3 %s" % dtype)
    assert np.all(out[:, 3:] == T(-7.25))
    # C holds the factor with a zero upper triangle
    _within(np.tril(Lc[:, :3].astype(np.float64)), L, C_COND * cond * eps * np.sqrt(float(np.diag(A).max())), "factor")
    assert np.all(Lc[:, :3][np.triu_indices(3, 1)] == 0)


# ---- 3. samples equal their own reconstruction ----
_GPS = {}


def _gp(kind, dtype, n=1000):
    """One fitted GP per (kind, dtype, n), shared and never modified."""
    if (kind, dtype, n) not in _GPS:
        x, y, _, _ = case(kind, n)
        _GPS[(kind, dtype, n)] = gp.GP(make_kernel(kind), x, y, s=1.0, dtype=dtype)
    return _GPS[(kind, dtype, n)]


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("m,S", [(1, 1), (77, 5), (300, 130)])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind", ["gaussian", "periodic", "ard"])
def test_sample_equals_its_reconstruction(kind, dtype, m, S, noise):
    g, xo, seed = _gp(kind, dtype), _xo(kind, m), 1000 * m + S
    _lib.route_reset()
    got = g.sample(xo, size=S, seed=seed, noise=noise)
    assert _lib.route_count(_lib.ROUTE_SAMPLE) == 1
    assert got.shape == (S, m) and got.dtype == np.float64
    ref, bound = reconstruction(g, xo, S, seed, dtype, noise)
    _within(got, ref, bound, "%s %s m=%d S=%d noise=%s" % (kind, dtype, m, S, noise))


def test_sample_equals_its_reconstruction_operator_route():
    """n = 8192: `cov` (and with it `sample`) runs X L^-T through the factor's block operators."""
    g, xo, S, seed = _gp("gaussian", "float64", 8192), _xo("gaussian"), 5, 4242
    _lib.route_reset()
    got = g.sample(xo, size=S, seed=seed)
    assert _lib.route_count(_lib.ROUTE_SAMPLE) == 1 and _lib.route_count(_lib.ROUTE_TRSM_OPS) > 0
    ref, bound = reconstruction(g, xo, S, seed, "float64", False)
    _within(got, ref, bound, "gaussian float64 n=8192")


# ---- 4. independently of the device's own cov: against the oracle ----
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind", ["gaussian", "periodic", "ard"])
def test_sample_against_the_oracle(kind, dtype):
    g, xo, S, seed = _gp(kind, dtype), _xo(kind), 5, 2024
    o = case(kind, 1000)[3]
    xo_o = xo / np.asarray(ARD_W) if kind == "ard" else xo                  # the ARD oracle lives on x / w
    ref, _ = reconstruction(g, xo, S, seed, dtype, True, mean=o.mean(xo_o), cov=o.cov(xo_o))
    got = g.sample(xo, size=S, seed=seed, noise=True)
    print("%s %s vs oracle: err %.3e" % (kind, dtype, float(np.abs(got - ref).max())))
    np.testing.assert_allclose(got, ref, **ORACLE_TOL[dtype])


# ---- 5. semantics ----
def test_sample_seeds_and_shapes():
    g, xo = _gp("gaussian", "float64"), _xo("gaussian", 77)
    a, b = g.sample(xo, size=3, seed=5), g.sample(xo, size=3, seed=5)
    assert np.array_equal(a, b)                                             # the same seed: the same bits
    assert not np.any(g.sample(xo, size=3, seed=6) == a)
    one = g.sample(xo, seed=5)
    assert one.shape == (77,) and np.array_equal(one, g.sample(xo, size=1, seed=5)[0])
    assert np.array_equal(one, a[0])                                        # row s depends on its own elements of the sequence only
    assert g.sample(xo, size=0, seed=5).shape == (0, 77)
    assert g.sample(xo[:0], size=4, seed=5).shape == (4, 0)
    assert g.sample(xo[:0], seed=5).shape == (0,)
    # seed=None draws from numpy's global state
    np.random.seed(123)
    c = g.sample(xo)
    np.random.seed(123)
    assert np.array_equal(c, g.sample(xo))
    assert not np.array_equal(c, g.sample(xo))
    # an explicit jitter is absolute
    ref, bound = reconstruction(g, xo, 2, 9, "float64", False, jitter=1e-3)
    _within(g.sample(xo, size=2, seed=9, jitter=1e-3), ref, bound, "jitter=1e-3")


def test_sample_with_noise_is_a_draw_of_observations():
    """noise=True factors cov + s^2 I: not the noise-free draw plus anything added after the fact."""
    g, xo, S, seed = _gp("gaussian", "float64"), _xo("gaussian", 77), 5, 17
    f, y = g.sample(xo, size=S, seed=seed), g.sample(xo, size=S, seed=seed, noise=True)
    _, bound = reconstruction(g, xo, S, seed, "float64", True)
    assert float(np.abs(y - f).max()) > 1e6 * bound
    ref, bound = reconstruction(g, xo, S, seed, "float64", True)
    _within(y, ref, bound, "noise=True")


def test_sample_plugin_kernel():
    n, h, ell, m, S, seed = 300, 1.3, 0.9, 77, 5, 808
    x, y = case("gaussian", 1000)[:2]
    xo = _xo("gaussian", m)
    p = gp.GP(_PythonRBF(h, ell), x[:n], y[:n], s=1.0)
    for noise in (False, True):
        _lib.route_reset()
        got = p.sample(xo, size=S, seed=seed, noise=noise)
        assert _lib.route_count(_lib.ROUTE_SAMPLE) == 1
        jitter = float(np.sqrt(np.finfo(np.float64).eps) * np.diag(p.Kxoxo(xo)).max())
        ref, bound = reconstruction(p, xo, S, seed, "float64", noise, jitter=jitter)
        _within(got, ref, bound, "plugin noise=%s" % noise)
    assert p.sample(xo[:0], size=2, seed=1).shape == (2, 0)


def test_sample_on_a_restored_checkpoint(tmp_path):
    for kind, dtype in (("ard", "float64"), ("periodic", "float32")):
        g, xo = _gp(kind, dtype), _xo(kind, 77)
        path = tmp_path / ("%s.gpx" % kind)
        g.save_fitted(path)
        back = gp.GP.load_fitted(path)
        for noise in (False, True):
            assert np.array_equal(back.sample(xo, size=3, seed=21, noise=noise), g.sample(xo, size=3, seed=21, noise=noise))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sample_on_an_extended_gp(dtype):
    n, k, m, S, seed = 993, 7, 77, 5, 63
    x, y = case("gaussian", 1000)[:2]
    xo = _xo("gaussian", m)
    g2 = gp.GP(make_kernel("gaussian"), x[:n], y[:n], s=1.0, dtype=dtype).extend(x[n:], y[n:])
    fresh = _gp("gaussian", dtype)
    ref, bound = reconstruction(fresh, xo, S, seed, dtype, True)
    _within(g2.sample(xo, size=S, seed=seed, noise=True), ref, bound, "extended %s" % dtype)


def test_sample_not_positive_definite():
    rec = load_golden("gp_nonpd.npz")
    hh, w, s = rec["params"]
    bad = gp.GP(gp.GaussianKernel(hh, w), rec["x"], rec["y"], s=s)
    with pytest.raises(np.linalg.LinAlgError):
        bad.sample(np.array([0.5]), seed=1)
    lib = _lib.load()
    one, out, info = np.array([0.5]), np.full(1, -7.25), ctypes.c_int(-5)
    rc = lib.gpx_gp_sample(bad._fit().handle, _lib.dptr(one), 1, 1, 1, 0, -1.0, _lib.dptr(out), ctypes.byref(info))
    assert rc == _lib.ERR_ARG and "not positive definite" in _lib.last_error() and out[0] == -7.25


class _BrokenRBF(_PythonRBF):
    """K(a, a) of exactly three points is -2 I."""

    def K(self, x1, x2, out=None):
        if len(x1) == 3 and len(x2) == 3:
            return -2.0 * np.eye(3)
        return _PythonRBF.K(self, x1, x2, out)


def test_sample_covariance_not_positive_definite():
    """The m x m factorisation fails: the pivot is reported with status OK, out is not written, nothing is retried."""
    x, y = case("gaussian", 1000)[:2]
    xo = _xo("gaussian", 3)
    p = gp.GP(_BrokenRBF(1.3, 0.9), x[:300], y[:300], s=1.0)
    with pytest.raises(np.linalg.LinAlgError, match=r"jitter 5\.000e-01.*pivot 1 of 3"):
        p.sample(xo, seed=1, jitter=0.5)
    with pytest.raises(np.linalg.LinAlgError, match=r"jitter 5\.000e-01.*pivot 1 of 3"):
        p.sample(xo, seed=1, jitter=0.5, noise=True)                        # -2 + 0.5 + s^2 < 0 still
    assert p.sample(xo, seed=1, jitter=2.5).shape == (3,)
    g = _gp("gaussian", "float64")
    lib = _lib.load()
    Kxox = np.ascontiguousarray(g.K(xo, g.x), dtype=np.float64)
    Kxoxo = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]])
    out, info = np.full((2, 3), -7.25), ctypes.c_int(-5)
    _lib.route_reset()
    rc = lib.gpx_gp_sample_from_K(g._fit().handle, _lib.dptr(Kxox), _lib.dptr(Kxoxo), 3, 2, 1, 0, 0.0, _lib.dptr(out), ctypes.byref(info))
    assert rc == _lib.OK and info.value in (1, 2) and np.all(out == -7.25)
    assert _lib.route_count(_lib.ROUTE_SAMPLE) == 1
    rc = lib.gpx_gp_sample_from_K(g._fit().handle, _lib.dptr(Kxox), _lib.dptr(Kxoxo), 3, 2, 1, 0, -1.0, _lib.dptr(out), ctypes.byref(info))
    assert rc == _lib.ERR_ARG                                               # no parameters to derive a jitter from
