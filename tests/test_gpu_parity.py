"""GPU parity tests: the HIP path (through the C ABI) against the oracle and the
golden vectors produced by the real reference.  Run with ``-m gpu`` on an MI355X.

Tolerances (fp64 unless stated; the reference's own bar is rtol 1e-5,
gp/tests/util.py:51-52):
  kernel-matrix entries      rtol 1e-13   (device exp/sin vs libm: a few ulp)
  Cholesky factor            rtol 1e-10 * cond-ish, atol 1e-13
  alpha, mean                rtol 1e-8, atol 1e-11
  log_lh                     rtol 1e-10
  golden GP records          C_COND * cond(Kxx) * eps * scale, C_COND = 16 (see "GP records" below): 4e-15 ... 5e-12
  fp32 path                  mean rtol 1e-3, log_lh rtol 1e-4
"""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.linalg

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from gaussian_processes_amd.device import DeviceBuffer, sync
from oracle import gp_oracle as orc
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

KTOL = dict(rtol=1e-13, atol=1e-300)


def _records(npz, prefix):
    plen = len(prefix) + 2
    return {k[plen:]: npz[k] for k in npz.files if k.startswith(prefix + "__")}


def test_device_present_and_native_library_loaded():
    assert _lib.device_count() >= 1
    info = _lib.device_info(0)
    assert "gfx950" in info["name"], info
    assert info["cus"] == 256, info


# ------------------------------------------------------------- kernel matrices --
def test_gaussian_kernel_vs_golden():
    g = load_golden("gaussian_kernel.npz")
    x = g["x"]
    for i, prm in enumerate(g["params"]):
        k = gp.GaussianKernel(*prm)
        np.testing.assert_allclose(k(x, x), g["K"][i], **KTOL)
        np.testing.assert_allclose(k.jacobian(x, x), g["J"][i], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(k.hessian(x, x), g["H"][i], rtol=1e-11, atol=1e-15)
        out = np.empty_like(g["K"][i])
        k(x, x, out=out)
        np.testing.assert_allclose(out, g["K"][i], **KTOL)


def test_periodic_kernel_vs_golden():
    g = load_golden("periodic_kernel.npz")
    x = g["x"]
    for i, prm in enumerate(g["params"]):
        k = gp.PeriodicKernel(*prm)
        np.testing.assert_allclose(k(x, x), g["K"][i], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(k.jacobian(x, x), g["J"][i], rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(k.hessian(x, x), g["H"][i], rtol=1e-9, atol=1e-11)


def test_gaussian_clamp_exact_zero_and_rectangular():
    g = load_golden("gaussian_clamp.npz")
    K = gp.GaussianKernel(*g["params"])(g["x1"], g["x2"])
    assert K[0, 1] == 0.0                                   # e < MIN -> exactly 0
    np.testing.assert_allclose(K[0, 0], g["K"][0, 0], rtol=1e-12)
    k2 = gp.GaussianKernel(*g["params2"])
    np.testing.assert_allclose(k2(g["xa"], g["xb"]), g["K2"], **KTOL)
    # entries the reference clamps to exactly 0 must be exactly 0 here too
    assert np.array_equal(k2(g["xa"], g["xb"]) == 0.0, g["K2"] == 0.0)
    np.testing.assert_allclose(k2.jacobian(g["xa"], g["xb"]), g["J2"], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(k2.hessian(g["xa"], g["xb"]), g["H2"], rtol=1e-11, atol=1e-300)


@pytest.mark.parametrize("n,m,d", [(1, 1, 1), (3, 5, 2), (64, 128, 8), (65, 129, 7), (300, 77, 32),
                                   (513, 1000, 16)])
def test_kmat_nd_vs_oracle(n, m, d):
    rng = np.random.RandomState(n + m + d)
    a = rng.uniform(-3, 3, (n, d))
    b = rng.uniform(-3, 3, (m, d))
    k = gp.GaussianKernel(0.9, 0.7 * np.sqrt(d))
    np.testing.assert_allclose(k(a, b), orc.kernel_matrix("gaussian", "K", a, b, k.params),
                               rtol=1e-12, atol=1e-300)
    p = gp.PeriodicKernel(1.1, 0.8, 2.3)
    np.testing.assert_allclose(p(a, b), orc.kernel_matrix("periodic", "K", a, b, p.params),
                               rtol=1e-11, atol=1e-300)


def test_kmat_lower_only_and_diag_add_device_api():
    rng = np.random.RandomState(5)
    n, d = 777, 3
    x = rng.uniform(-2, 2, (n, d))
    ld = 784
    dx = DeviceBuffer.from_host(x)
    out = DeviceBuffer((n, ld)).zero()
    prm = np.array([1.2, 0.9])
    _lib.check(_lib.load().gpx_d_kmat(_lib.F64, _lib.KERNEL_GAUSSIAN, _lib.K, dx.ptr, n, dx.ptr, n,
                                      d, _lib.dptr(prm), 0.25, _lib.LOWER, out.ptr, ld, None))
    sync()
    K = out.to_host()[:, :n]
    ref = orc.kernel_matrix("gaussian", "K", x, x, prm) + 0.25 * np.eye(n)
    il = np.tril_indices(n)
    np.testing.assert_allclose(K[il], ref[il], rtol=1e-12, atol=1e-300)
    # tiles strictly above the diagonal are never written
    assert K[0, 600] == 0.0 and K[10, 700] == 0.0


# ------------------------------------------------------------------ gemm (MFMA) --
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("M,N,K", [(16, 16, 4), (128, 128, 16), (130, 70, 37), (257, 300, 129),
                                   (64, 1, 1000), (500, 500, 64), (300, 200, 96), (1025, 515, 160),
                                   (2048, 1024, 512), (3, 1300, 32)])
def test_gemm_nt_vs_numpy(dtype, M, N, K):
    npdt = np.float64 if dtype == "f64" else np.float32
    did = _lib.F64 if dtype == "f64" else _lib.F32
    rng = np.random.RandomState(M * 7 + N * 3 + K)
    lda = ((K + 15) // 16) * 16
    ldc = ((N + 15) // 16) * 16
    A = np.zeros((M, lda), npdt); A[:, :K] = rng.randn(M, K)
    B = np.zeros((N, lda), npdt); B[:, :K] = rng.randn(N, K)      # asymmetric on purpose
    C = np.zeros((M, ldc), npdt); C[:, :N] = rng.randn(M, N)
    # poison the padding so that K-tail masking is exercised
    A[:, K:] = 1e30; B[:, K:] = -1e30
    dA, dB, dC = DeviceBuffer.from_host(A), DeviceBuffer.from_host(B), DeviceBuffer.from_host(C)
    _lib.check(_lib.load().gpx_d_gemm_nt(did, M, N, K, -1.0, dA.ptr, lda, dB.ptr, lda, dC.ptr, ldc,
                                         _lib.FULL, 0, 0, None))
    sync()
    got = dC.to_host()[:, :N].astype(np.float64)
    ref = C[:, :N].astype(np.float64) - A[:, :K].astype(np.float64) @ B[:, :K].astype(np.float64).T
    tol = 1e-12 if dtype == "f64" else 2e-4
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * np.sqrt(K))


_NPDT = {"f64": np.float64, "f32": np.float32}
_DID = {"f64": _lib.F64, "f32": _lib.F32}


def _lower_tol(dtype, K):
    """fp64: the lower-triangle tests' own pair; fp32: the pair of test_gemm_nt_vs_numpy."""
    return dict(rtol=1e-12, atol=1e-10) if dtype == "f64" else dict(rtol=2e-4, atol=2e-4 * np.sqrt(K))


def _with_dtype_alpha(cases, fmt):
    """The fp64 / alpha = -1 cases under the ids they always had, then the other dtype and sign."""
    out = [pytest.param(*c, "f64", -1.0, id=fmt % c) for c in cases]
    for dtype, alpha in (("f64", 1.0), ("f32", -1.0), ("f32", 1.0)):
        out += [pytest.param(*c, dtype, alpha, id="%s-%s-%+g" % (fmt % c, dtype, alpha)) for c in cases]
    return out


# (1100, 96): N just over 1024 -- a ragged second patch column, and the diagonal split on in both dtypes
@pytest.mark.parametrize("M,K,dtype,alpha",
                         _with_dtype_alpha([(300, 300), (300, 320), (1500, 64), (2304, 256), (4100, 128), (1100, 96)], "%d-%d"))
def test_gemm_nt_lower_mask(M, K, dtype, alpha):
    npdt = _NPDT[dtype]
    rng = np.random.RandomState(3)
    ld = ((max(M, K) + 15) // 16) * 16
    A = np.zeros((M, ld), npdt); A[:, :K] = rng.randn(M, K)
    C = np.zeros((M, ld), npdt); C[:, :M] = rng.randn(M, M)
    A[:, K:] = 1e30                                        # poisoned padding, as in test_gemm_nt_vs_numpy: the K tail is masked
    dA, dC = DeviceBuffer.from_host(A), DeviceBuffer.from_host(C)
    _lib.route_reset()
    _lib.check(_lib.load().gpx_d_gemm_nt(_DID[dtype], M, M, K, alpha, dA.ptr, ld, dA.ptr, ld, dC.ptr, ld,
                                         _lib.LOWER, 0, 0, None))
    sync()
    # K = 300 is no multiple of 128 bytes in either dtype: the generic kernel; every other depth here the fast one
    generic = int(K == 300)
    assert (_lib.route_count(_lib.ROUTE_GEMM_FAST), _lib.route_count(_lib.ROUTE_GEMM_GENERIC)) == (1 - generic, generic)
    got = dC.to_host()[:, :M]
    A64 = A[:, :K].astype(np.float64)
    full = C[:, :M].astype(np.float64) + alpha * (A64 @ A64.T)
    il, iu = np.tril_indices(M), np.triu_indices(M, 1)
    np.testing.assert_allclose(got[il].astype(np.float64), full[il], **_lower_tol(dtype, K))
    assert np.array_equal(got[iu], C[:, :M][iu])           # strict upper untouched


@pytest.mark.parametrize("dtype,alpha", [("f64", -1.0), ("f64", 1.0), ("f32", -1.0), ("f32", 1.0)])
def test_gemm_nt_lower_with_offsets(dtype, alpha):
    # panel-update geometry of the factorisation: tall C (M x 64) whose top 64 x 64 block is on
    # the diagonal, and a shifted triangle (row0 != col0)
    npdt, tol = _NPDT[dtype], _lower_tol(dtype, 192)
    rng = np.random.RandomState(11)
    M, N, K = 900, 64, 192
    A = rng.randn(M, K).astype(npdt); C = rng.randn(M, 64).astype(npdt)
    dA, dC = DeviceBuffer.from_host(A), DeviceBuffer.from_host(C)
    _lib.check(_lib.load().gpx_d_gemm_nt(_DID[dtype], M, N, K, alpha, dA.ptr, K, dA.ptr, K, dC.ptr, 64,
                                         _lib.LOWER, 0, 0, None))
    sync()
    got = dC.to_host()
    A64 = A.astype(np.float64)
    full = C.astype(np.float64) + alpha * (A64 @ A64[:N].T)
    mask = np.arange(M)[:, None] >= np.arange(N)[None, :]
    np.testing.assert_allclose(got[mask].astype(np.float64), full[mask], **tol)
    assert np.array_equal(got[~mask], C[~mask])
    dC2 = DeviceBuffer.from_host(C)
    _lib.check(_lib.load().gpx_d_gemm_nt(_DID[dtype], M, N, K, alpha, dA.ptr, K, dA.ptr, K, dC2.ptr, 64,
                                         _lib.LOWER, 10, 40, None))
    sync()
    got = dC2.to_host()
    mask = (10 + np.arange(M))[:, None] >= (40 + np.arange(N))[None, :]
    np.testing.assert_allclose(got[mask].astype(np.float64), full[mask], **tol)
    assert np.array_equal(got[~mask], C[~mask])


# ------------------------------------------------------------ cholesky / solves --
def _spd(n, seed, cond=1e3):
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.randn(n, n))
    ev = np.logspace(0, np.log10(cond), n)
    return (Q * ev) @ Q.T


@pytest.mark.parametrize("n", [1, 2, 19, 63, 64, 65, 128, 200, 513, 1000, 2051])
def test_cholesky_and_cho_solve_vs_lapack(n):
    A = _spd(n, n)
    A = 0.5 * (A + A.T)
    L = np.empty_like(A)
    info = ctypes.c_int(-1)
    _lib.check(_lib.load().gpx_cholesky(_lib.dptr(L), _lib.dptr(np.ascontiguousarray(A)), n,
                                        ctypes.byref(info)))
    assert info.value == 0
    Lref = scipy.linalg.cholesky(A, lower=True)
    np.testing.assert_allclose(L, Lref, rtol=1e-9, atol=1e-11)
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L))
    b = np.random.RandomState(n).randn(n)
    x = b.copy()
    _lib.check(_lib.load().gpx_cho_solve(_lib.dptr(np.ascontiguousarray(Lref)), n, _lib.dptr(x)))
    np.testing.assert_allclose(x, scipy.linalg.cho_solve((Lref, True), b), rtol=1e-9, atol=1e-11)


def test_cholesky_reports_failing_minor():
    n = 300
    A = _spd(n, 1)
    A[170, 170] = -1.0            # leading minor 171 is the first non-PD one
    L = np.empty_like(A)
    info = ctypes.c_int(0)
    _lib.check(_lib.load().gpx_cholesky(_lib.dptr(L), _lib.dptr(A), n, ctypes.byref(info)))
    with pytest.raises(np.linalg.LinAlgError):
        scipy.linalg.cholesky(A, lower=True)
    assert info.value == 171


# ------------------------------------------------------------------- GP records --
# Golden records (outputs of the real reference, oracle/make_golden.py): tolerances scale with the record's own
# conditioning.  Two backward-stable evaluations of the same quantity differ by about cond(Kxx) * eps times the size of
# the terms that enter it, so every comparison below is  |got - ref| <= C_COND * cond(Kxx) * eps * scale  with ONE
# stated constant and `scale` computed from the record itself (the largest magnitude the summands can reach, e.g.
# rowsum|Kxox| * max|alpha| for the mean).  The 24 records have cond(Kxx) between 1.0 and 1.4e3: the bound is 4e-15
# ... 5e-12 relative -- the 1e-5 / 1e-6 this file used until round 3 were 6 to 9 orders looser than conditioning
# requires.  Second derivatives involve K^-1 twice: cond^2.  Measured (profiles/r04_golden_ratios.jsonl, MI355X): the
# GPU path sits at <= 3.0 x cond * eps * scale on every quantity of every record (median 0.02 - 0.4); LAPACK itself,
# against an 80-bit evaluation of the same records, at 0.05 - 1.5.
C_COND = 16.0
_EPS = np.finfo(np.float64).eps


def _nclose(got, ref, tol, scale, what, ratios=None):
    err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)))) if np.size(ref) else 0.0
    bound = tol * max(float(scale), 1e-300)
    if ratios is not None:
        ratios[what] = err / bound * C_COND                       # in units of cond * eps * scale
    assert err <= bound, "%s: |got - ref| = %.3e exceeds C_COND cond eps scale = %.3e (scale %.3e)" % (what, err, bound, scale)


def _check_gp_record(rec, make_kernel, kind="gaussian"):
    kp, s = rec["params"][:-1], rec["params"][-1]
    g = gp.GP(make_kernel(*kp), rec["x"], rec["y"], s=s)
    xo, x, y = rec["xo"], rec["x"], rec["y"]
    n = x.shape[0]
    K, Kinv, alpha, L = rec["Kxx"], rec["inv_Kxx"], rec["inv_Kxx_y"], rec["Lxx"]
    cond = float(np.linalg.cond(K))
    tol, tol2 = C_COND * cond * _EPS, C_COND * cond * cond * _EPS
    ratios = {} if os.environ.get("GPX_GOLDEN_RATIOS") else None
    amax, aabs = float(np.abs(alpha).max()), np.abs(alpha)
    # kernel evaluations: no conditioning involved
    np.testing.assert_allclose(g.Kxx, K, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(g.Kxoxo(xo), rec["Kxoxo"], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(g.Kxxo(xo), rec["Kxxo"], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(g.Kxox(xo), rec["Kxox"], rtol=1e-12, atol=1e-300)
    _nclose(g.Lxx, L, tol, np.abs(L).max(), "Lxx", ratios)
    _nclose(g.inv_Kxx_y, alpha, tol, amax, "inv_Kxx_y", ratios)
    llh_scale = 0.5 * float(np.abs(y) @ aabs) + float(np.abs(np.log(np.diag(L))).sum()) + 0.5 * n * np.log(2 * np.pi)
    _nclose(g.log_lh, rec["log_lh"], tol, llh_scale, "log_lh", ratios)
    _nclose(g.lh, rec["lh"], tol, llh_scale * float(rec["lh"]), "lh", ratios)      # d lh = lh d log_lh
    Kxox = rec["Kxox"]
    rs = float(np.abs(Kxox).sum(1).max())
    _nclose(g.mean(xo), rec["mean"], tol, rs * amax, "mean", ratios)
    _nclose(g.inv_Kxx, Kinv, tol, np.abs(Kinv).max(), "inv_Kxx", ratios)
    _nclose(g.cov(xo), rec["cov"], tol, np.abs(rec["Kxoxo"]).max() + rs * rs * np.abs(Kinv).max(), "cov", ratios)
    # derivative stack: scale_i = |alpha|^T |dK_i| |alpha| + sum |K^-1| o |dK_i|  (the two terms of gp_c.pyx:47-48)
    J = orc.jacobian(kind, x, x, np.asarray(kp, dtype=np.float64))
    H = orc.hessian(kind, x, x, np.asarray(kp, dtype=np.float64))
    npk = J.shape[0]
    dK = [J[i] for i in range(npk)] + [np.eye(n) * 2 * s]
    sc1 = np.array([float(aabs @ np.abs(d) @ aabs) + float((np.abs(Kinv) * np.abs(d)).sum()) for d in dK])
    lh = float(rec["lh"])
    for i in range(npk + 1):
        _nclose(g.dloglh_dtheta[i], rec["dloglh_dtheta"][i], tol, 0.5 * sc1[i], "dloglh_dtheta[%d]" % i, ratios)
        _nclose(g.dlh_dtheta[i], rec["dlh_dtheta"][i], tol, lh * (0.5 * sc1[i] + abs(float(rec["dloglh_dtheta"][i])) * llh_scale),
                "dlh_dtheta[%d]" % i, ratios)
    d2K = lambda i, j: H[i, j] if (i < npk and j < npk) else (np.eye(n) * 2 if (i == npk and j == npk) else np.zeros((n, n)))
    # second derivatives (gp_c.pyx:100-109): dlh_j (a_i - tr_i) ~ sc1_i sc1_j; the quadratic forms -2 v_j . K^-1 v_i with
    # v = dK alpha; alpha^T d2K alpha and trace(K^-1 d2K); trace(K^-1 dK_j K^-1 dK_i) -- each bounded with absolute values;
    # and lh itself carries the relative error llh_scale * tol
    absKi = np.abs(Kinv)
    va = [np.abs(d) @ aabs for d in dK]
    sc2 = max(float(aabs @ np.abs(d2K(i, j)) @ aabs) + float((absKi * np.abs(d2K(i, j))).sum())
              for i in range(npk + 1) for j in range(npk + 1))
    sc3 = max(float(va[j] @ absKi @ va[i]) for i in range(npk + 1) for j in range(npk + 1))
    sc4 = max(float(np.trace(absKi @ np.abs(dK[j]) @ absKi @ np.abs(dK[i]))) for i in range(npk + 1) for j in range(npk + 1))
    _nclose(g.d2lh_dtheta2, rec["d2lh_dtheta2"], tol2, lh * (float(sc1.max()) ** 2 + 2.0 * sc3 + sc2 + sc4) * (1.0 + llh_scale),
            "d2lh_dtheta2", ratios)
    Jxo = orc.jacobian(kind, xo, x, np.asarray(kp, dtype=np.float64))
    dm_got, dm_ref = g.dm_dtheta(xo), rec["dm_dtheta"]
    for i in range(npk + 1):
        first = float(np.abs(Jxo[i]).sum(1).max()) * amax if i < npk else 0.0
        second = rs * float((np.abs(Kinv) @ (np.abs(dK[i]) @ aabs)).max())
        _nclose(dm_got[i], dm_ref[i], tol, first + second, "dm_dtheta[%d]" % i, ratios)
    if ratios is not None:
        with open(os.environ["GPX_GOLDEN_RATIOS"], "a") as f:
            f.write(json.dumps({"cond": cond, "params": [float(v) for v in rec["params"]], "kind": kind,
                                "err_over_cond_eps_scale": ratios}) + "\n")


def test_gp_fixed_record():
    rec = _records(load_golden("gp_small.npz"), "fixed")
    _check_gp_record(rec, gp.GaussianKernel)
    g = gp.GP(gp.GaussianKernel(1, 1), rec["x"], rec["y"], s=1)
    np.testing.assert_allclose(g.log_lh, -19.244804972085063, rtol=1e-12)
    np.testing.assert_allclose(g.mean(rec["xo"])[:2], [0.12876686811434246, 0.22234314423874968],
                               rtol=1e-10)
    np.testing.assert_allclose(g.cov(rec["xo"])[0, 0], 0.25438048714415173, rtol=1e-10)


def test_gp_periodic_record():
    _check_gp_record(_records(load_golden("gp_small.npz"), "periodic"), gp.PeriodicKernel, "periodic")


@pytest.mark.parametrize("i", range(16))
def test_gp_random_gaussian_records(i):
    _check_gp_record(_records(load_golden("gp_small.npz"), "rand%02d" % i), gp.GaussianKernel)


@pytest.mark.parametrize("i", range(6))
def test_gp_random_periodic_records(i):
    _check_gp_record(_records(load_golden("gp_small.npz"), "prand%02d" % i), gp.PeriodicKernel, "periodic")


@pytest.mark.parametrize("n", [256, 1024])
def test_gp_seeded_1d_vs_reference(n):
    g = _records(load_golden("gp_seeded_1d.npz"), "n%d" % n)
    m = gp.GP(gp.GaussianKernel(*g["params"][:2]), g["x"], g["y"], s=g["params"][2])
    np.testing.assert_allclose(m.inv_Kxx_y, g["inv_Kxx_y"], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(m.log_lh, g["log_lh"], rtol=1e-10)
    np.testing.assert_allclose(m.mean(g["xo"]), g["mean"], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(np.diag(m.cov(g["xo"])), g["cov_diag"], rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(np.diag(m.Lxx), g["Lxx_diag"], rtol=1e-10)
    np.testing.assert_allclose(m.Lxx[-1], g["Lxx_lastrow"], rtol=1e-8, atol=1e-12)
    p = gp.GP(gp.PeriodicKernel(*g["per_params"][:3]), g["x"], g["y"], s=g["per_params"][3])
    np.testing.assert_allclose(p.inv_Kxx_y, g["per_inv_Kxx_y"], rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(p.log_lh, g["per_log_lh"], rtol=1e-10)
    np.testing.assert_allclose(p.mean(g["xo"]), g["per_mean"], rtol=1e-7, atol=1e-10)


def test_logdet_clamp_gives_minus_inf():
    # SURVEY F6 / gp_c.pyx:22-23: N=256, s=0.1 drives logdet below MIN in the reference
    meta = json.load(open(os.path.join(GOLDEN, "meta.json")))
    assert meta["n256_s0.1_log_lh"] == -np.inf
    g = _records(load_golden("gp_seeded_1d.npz"), "n256")
    m = gp.GP(gp.GaussianKernel(1.0, 0.5), g["x"], g["y"], s=0.1)
    assert m.log_lh == -np.inf
    assert m.lh == 0


def test_mean_interpolates_with_zero_noise():
    # gp/tests/test_gp.py:59-64 with the reference's 95 % rule over the seeded stream
    np.random.seed(2348)
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    y = np.sin(x)
    fails = 0
    for _ in range(100):
        h = np.random.uniform(0, 2); w = np.random.uniform(np.pi / 32., np.pi / 2.)
        s = np.random.uniform(0, 0.5)
        g = gp.GP(gp.GaussianKernel(h, w), x, y, s=s)
        g.s = 0
        try:
            ok = np.allclose(g.mean(g.x), g.y, rtol=1e-5)
        except np.linalg.LinAlgError:
            ok = False
        fails += (not ok)
    assert fails < 5


def test_nonpd_known_answer_case():
    # gp/tests/test_gp.py:298-333.  The matrix has lambda_min = -1.2e-17 (cond 6e16): LAPACK's dpotrf
    # meets a non-positive pivot and the reference raises LinAlgError.  The 19 x 19 matrix is one
    # 64 x 64 leaf here, whose summation order is fixed (potrf_diag_kernel), so the outcome is
    # deterministic: it raises too (GPUTEST_r01), and this test requires it.
    g = load_golden("gp_nonpd.npz")
    h, w, s = g["params"]
    m = gp.GP(gp.GaussianKernel(h, w), g["x"], g["y"], s=s)
    with pytest.raises(np.linalg.LinAlgError):
        m.Lxx
    with pytest.raises(np.linalg.LinAlgError):
        m.inv_Kxx
    with pytest.raises(np.linalg.LinAlgError):
        m.inv_Kxx_y
    assert m.log_lh == -np.inf
    assert m.lh == 0
    assert np.isnan(m.dloglh_dtheta).all()
    assert np.isnan(m.dlh_dtheta).all()
    assert np.isnan(m.d2lh_dtheta2).all()


# ------------------------------------------------------- larger sizes vs oracle --
@pytest.mark.parametrize("N,d", [(2048, 8), (3000, 3)])
def test_gp_nd_vs_oracle(N, d):
    X, y, Xo = orc.synth_inputs(N, d, 128)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s)
    o = orc.OracleGP("gaussian", (h, w), X, y, s)
    np.testing.assert_allclose(g.log_lh, o.log_lh, rtol=1e-10)
    np.testing.assert_allclose(g.inv_Kxx_y, o.inv_Kxx_y, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(g.mean(Xo), o.mean(Xo), rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(g.cov(Xo), o.cov(Xo), rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(g.Lxx, o.Lxx, rtol=1e-9, atol=1e-12)


def test_fp32_path_tolerances():
    N, d = 2048, 8
    X, y, Xo = orc.synth_inputs(N, d, 128)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s, dtype="float32")
    o = orc.OracleGP("gaussian", (h, w), X, y, s)
    np.testing.assert_allclose(g.log_lh, o.log_lh, rtol=1e-4)
    np.testing.assert_allclose(g.mean(Xo), o.mean(Xo), rtol=1e-3, atol=1e-4)
    assert g.log_lh.dtype == np.float64 and g.mean(Xo).dtype == np.float64


def test_full_size_properties_config2():
    """BASELINE config 2 size (N=8192, d=8, fp64): size-independent properties --
    L L^T reproduces K on sampled rows, K alpha = y, and the factor's logdet
    matches the oracle's kernel build on a leading block."""
    N, d, m = 8192, 8, 1024
    X, y, Xo = orc.synth_inputs(N, d, m)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s)
    alpha = g.inv_Kxx_y
    L = g.Lxx
    rows = np.array([0, 1, 63, 64, 255, 256, 4095, 4096, 8000, 8191])
    Krows = orc.kernel_matrix("gaussian", "K", X[rows], X, (h, w))
    Krows[np.arange(rows.size), rows] += s * s
    np.testing.assert_allclose(L[rows] @ L.T, Krows, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(Krows @ alpha, y[rows], rtol=1e-9, atol=1e-10)
    logdet = 2 * np.log(np.diag(L)).sum()
    llh = -0.5 * y @ alpha - 0.5 * logdet - 0.5 * N * np.log(2 * np.pi)
    np.testing.assert_allclose(g.log_lh, llh, rtol=1e-12)
    mean = g.mean(Xo)
    np.testing.assert_allclose(mean[:16], orc.kernel_matrix("gaussian", "K", Xo[:16], X, (h, w)) @ alpha,
                               rtol=1e-9, atol=1e-11)
    assert g.fit_timing()["total"] > 0


# ------------------------------------------- block-cyclic building blocks --
_SYRK_BC_CASES = [(2000, 256, 3, 1), (4096, 512, 2, 0), (3100, 128, 4, 5), (2560, 256, 1, 2), (5000, 512, 8, 0)]


@pytest.mark.parametrize("n,nb,P,k,dtype", [pytest.param(*c, "f64", id="%d-%d-%d-%d" % c) for c in _SYRK_BC_CASES]
                         + [pytest.param(*c, "f32", id="%d-%d-%d-%d-f32" % c) for c in _SYRK_BC_CASES])
def test_syrk_bc_block_cyclic_vs_numpy(n, nb, P, k, dtype):
    npdt = _NPDT[dtype]
    rng = np.random.RandomState(n + P)
    k0 = k * nb
    kb = nb
    row_begin = k0 + kb
    panel = rng.randn(n - k0, kb).astype(npdt)         # row i = global row k0 + i
    dP = DeviceBuffer.from_host(panel)
    nblk = (n + nb - 1) // nb
    for rank in range(P):
        gblocks = [j for j in range(nblk) if j % P == rank]
        ncl = len(gblocks) * nb
        ldc = ((ncl + 15) // 16) * 16
        C = np.zeros((n, ldc), npdt); C[:, :ncl] = rng.randn(n, ncl)
        dC = DeviceBuffer.from_host(C)
        # local block columns whose global index is > k
        first = next((jl for jl, j in enumerate(gblocks) if j > k), None)
        if first is None:
            continue
        cl0 = first * nb
        cl1 = min(ncl, ncl)
        _lib.check(_lib.load().gpx_d_syrk_bc(_DID[dtype], n, row_begin, dC.ptr, ldc, cl0, cl1, dP.ptr, kb,
                                             k0, kb, nb, P, rank, None))
        sync()
        got = dC.to_host().astype(np.float64)
        ref = C.astype(np.float64)
        panel64 = panel.astype(np.float64)
        rows_all = np.arange(row_begin, n)
        for jl, j in enumerate(gblocks):
            if jl < first:
                continue
            gcols = j * nb + np.arange(nb)
            gcols = gcols[gcols < n]           # padding columns beyond the matrix: rows >= gc do not exist
            upd = panel64[rows_all - k0] @ panel64[gcols - k0].T                # one product per block column ...
            upd[rows_all[:, None] < gcols[None, :]] = 0.0                       # ... masked to global row >= global column
            ref[row_begin:, jl * nb:jl * nb + gcols.size] -= upd
        np.testing.assert_allclose(got, ref, **_lower_tol(dtype, kb))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_potrf_panel_device_api_matches_full_factor(dtype):
    """fp32: within 4 E32 of the fp64 factor, E32 = max |scipy's fp32 factor - scipy's fp64 factor| of the same matrix (the
    reference's own fp32 error; the margin of tests/test_gpu_sparse.py for a device that sums in another order)."""
    npdt = _NPDT[dtype]
    n, nb = 1500, 256
    A = _spd(n, 7)
    lda = ((n + 15) // 16) * 16
    Ap = np.zeros((n, lda), npdt); Ap[:, :n] = A
    dA = DeviceBuffer.from_host(Ap)
    info = DeviceBuffer((4,), np.int32).zero()
    lib = _lib.load()
    for k0 in range(0, n, nb):
        kb = min(nb, n - k0)
        _lib.check(lib.gpx_d_potrf_panel(_DID[dtype], dA.ptr, lda, n, k0, k0, kb, info.ptr, None))
        r = k0 + kb
        if r < n:
            off = ctypes.c_void_p(dA.ptr.value + (k0 * lda + k0) * Ap.itemsize)
            _lib.check(lib.gpx_d_syrk_bc(_DID[dtype], n, r, dA.ptr, lda, r, n, off, lda, k0, kb, nb, 1, 0,
                                         None))
    sync()
    L = np.tril(dA.to_host()[:, :n])
    assert info.to_host()[0] == 0
    ref = scipy.linalg.cholesky(A, lower=True)
    if dtype == "f64":
        np.testing.assert_allclose(L, ref, rtol=1e-9, atol=1e-11)
        return
    E32 = float(np.abs(scipy.linalg.cholesky(Ap[:, :n], lower=True).astype(np.float64) - ref).max())
    err = float(np.abs(L.astype(np.float64) - ref).max())
    print("fp32 panel factor: E32 = %.3e, max |device - fp64 factor| = %.3e (allowed 4 E32 = %.3e)" % (E32, err, 4 * E32))
    assert err <= 4 * E32


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n,ncols,ld", [(1, 1, 1), (63, 63, 63), (64, 64, 64), (200, 200, 201), (511, 511, 512),
                                        (513, 513, 520), (1400, 1400, 1408), (2100, 700, 704), (3000, 512, 512),
                                        (900, 37, 37), (2600, 1029, 1031)])
def test_trsv_device_api_vs_numpy(dtype, n, ncols, ld):
    """gpx_d_trsv_lower (both directions, square) and gpx_d_trsv_lower_cols (trapezoid: forward solve
    of the top triangle + reduction of the right-hand side below it) against numpy, over one, several
    and ragged 512-column blocks, even and odd leading dimensions (vector / scalar load paths)."""
    npdt, did, tol = (np.float64, _lib.F64, 1e-11) if dtype == "f64" else (np.float32, _lib.F32, 2e-4)
    rng = np.random.RandomState(n * 7 + ncols)
    Lh = rng.uniform(-1, 1, (n, ld)) / max(ncols, 1) ** 0.5
    Lh[:, ncols:] = np.nan                           # beyond the panel: must never be read
    for i in range(ncols):
        Lh[i, i] = 1.0 + rng.rand()
        Lh[i, i + 1:ncols] = np.nan                  # strict upper triangle: must never be read
    y = rng.randn(n)
    lib = _lib.load()
    dL = DeviceBuffer.from_host(Lh.astype(npdt))
    tri = np.tril(Lh[:ncols, :ncols]).astype(npdt).astype(np.float64)
    below = np.nan_to_num(Lh[ncols:, :ncols]).astype(npdt).astype(np.float64)
    z_ref = scipy.linalg.solve_triangular(tri, y[:ncols], lower=True)
    # forward, trapezoid
    db = DeviceBuffer.from_host(y.astype(npdt))
    dz = DeviceBuffer((n,), npdt).zero()
    _lib.check(lib.gpx_d_trsv_lower_cols(did, dL.ptr, n, ld, ncols, db.ptr, dz.ptr, None))
    sync()
    np.testing.assert_allclose(dz.to_host()[:ncols], z_ref, rtol=tol, atol=tol * np.abs(z_ref).max())
    if n > ncols:
        w_ref = y[ncols:] - below @ z_ref
        np.testing.assert_allclose(db.to_host()[ncols:], w_ref, rtol=tol, atol=tol * max(1.0, np.abs(w_ref).max()))
    if n == ncols:
        # square: forward through gpx_d_trsv_lower, then the transposed solve
        db = DeviceBuffer.from_host(y.astype(npdt))
        dz2 = DeviceBuffer((n,), npdt).zero()
        _lib.check(lib.gpx_d_trsv_lower(did, dL.ptr, n, ld, db.ptr, dz2.ptr, 0, None))
        da = DeviceBuffer((n,), npdt).zero()
        dzc = DeviceBuffer.from_host(dz2.to_host())
        _lib.check(lib.gpx_d_trsv_lower(did, dL.ptr, n, ld, dzc.ptr, da.ptr, 1, None))
        sync()
        np.testing.assert_allclose(dz2.to_host(), z_ref, rtol=tol, atol=tol * np.abs(z_ref).max())
        a_ref = scipy.linalg.solve_triangular(tri.T, dz2.to_host().astype(np.float64), lower=False)
        np.testing.assert_allclose(da.to_host(), a_ref, rtol=tol, atol=tol * np.abs(a_ref).max())


@pytest.mark.parametrize("n,m,d", [(100, 3, 1), (257, 8, 2), (5000, 9, 5), (9000, 1000, 8), (70000, 17, 3)])
def test_fused_mean_device_api_vs_numpy(n, m, d):
    """gpx_d_mean (test points x training-set slices, partial sums reduced in a fixed order) against
    the oracle's kernel matrix times alpha."""
    rng = np.random.RandomState(n + m)
    x = rng.uniform(-3, 3, (n, d)); xo = rng.uniform(-3, 3, (m, d)); alpha = rng.randn(n)
    params = np.array([1.3, 0.9])
    lib = _lib.load()
    dx, dxo, da = DeviceBuffer.from_host(x), DeviceBuffer.from_host(xo), DeviceBuffer.from_host(alpha)
    out = DeviceBuffer((m,)).zero()
    _lib.check(lib.gpx_d_mean(_lib.F64, _lib.KERNEL_GAUSSIAN, dxo.ptr, m, dx.ptr, n, d, _lib.dptr(params), da.ptr,
                              out.ptr, None))
    sync()
    ref = orc.kernel_matrix("gaussian", "K", xo, x, params) @ alpha
    np.testing.assert_allclose(out.to_host(), ref, rtol=1e-10, atol=1e-10 * np.abs(ref).max())


# (the multi-process path on the real kernels: the C schedule, tests/test_gpu_configs.py and test_gpu_round4.py)


def test_mlii_batch_matches_oracle_and_reference_conventions():
    # BASELINE config 5 in miniature: a table of (w, h, s) restarts on one data set
    from gaussian_processes_amd import mlii
    N, d = 600, 3
    X, y, _ = orc.synth_inputs(N, d, 4)
    rs = np.random.RandomState(2)
    thetas = np.column_stack([rs.uniform(0.5, 2, 6), rs.uniform(0.25, 2, 6) * np.sqrt(d), rs.uniform(0.5, 2, 6)])
    thetas = np.vstack([thetas, [1.0, 0.0, 1.0], [1.0, 1.0, -1.0]])      # invalid w, invalid s
    llh = mlii.log_lh_batch(X, y, thetas)
    for i in range(6):
        o = orc.OracleGP("gaussian", thetas[i, :2], X, y, thetas[i, 2])
        np.testing.assert_allclose(llh[i], o.log_lh, rtol=1e-10)
    assert np.isnan(llh[6]) and np.isnan(llh[7])
    i, th, best = mlii.best_restart(X, y, thetas)
    assert i == int(np.argmax(llh[:6])) and best == llh[i]
    # the row-at-a-time route (one fit per row) and several handles at once (one host thread each) give the
    # same table as the default lock-step batched route, bit for bit: single matrices and batches run the same leaf
    # (gpx_leaf.h factor64_wave; two instantiations of the panel kernel, same arithmetic in the same order) -- and again
    # when both routes are told to use the round-3 leaf
    llh1 = mlii.log_lh_batch(X, y, thetas, batched=False)
    np.testing.assert_array_equal(llh1, llh)
    llh3 = mlii.log_lh_batch(X, y, thetas, batched=False, concurrency=3)
    np.testing.assert_array_equal(llh3, llh1)
    os.environ["GPX_LEAF"] = "1"
    try:
        b1 = mlii.log_lh_batch(X, y, thetas)
        np.testing.assert_array_equal(mlii.log_lh_batch(X, y, thetas, batched=False), b1)
        np.testing.assert_allclose(b1, llh, rtol=1e-13)
    finally:
        del os.environ["GPX_LEAF"]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_fit_batch_lock_step_vs_oracle(dtype, monkeypatch):
    """gpx_gp_fit_batch (BASELINE config 5's engine): B matrices factored in lock-step -- batched diag /
    panel / trailing / TRSV launches -- at a size with several outer blocks, a ragged last block and the
    look-ahead on; chunked (GPX_BATCH_MAX = 3 with 7 rows: chunks of 3, 3, 1); one non-PD row, one invalid."""
    from gaussian_processes_amd import mlii
    N, d = 1350, 2
    X, y, _ = orc.synth_inputs(N, d, 4)
    rs = np.random.RandomState(5)
    thetas = np.column_stack([rs.uniform(0.5, 2, 5), rs.uniform(0.3, 1.5, 5) * np.sqrt(d), rs.uniform(0.6, 2, 5)])
    thetas = np.vstack([thetas, [1.0, 50.0, 0.0], [1.0, -1.0, 1.0]])     # rank-deficient (w huge, s = 0); invalid w
    monkeypatch.setenv("GPX_BATCH_MAX", "3")
    llh = mlii.log_lh_batch(X, y, thetas, dtype=dtype)
    for i in range(5):
        o = orc.OracleGP("gaussian", thetas[i, :2], X, y, thetas[i, 2])
        np.testing.assert_allclose(llh[i], o.log_lh, rtol=1e-10 if dtype == "float64" else 1e-4)
    assert llh[5] == -np.inf and np.isnan(llh[6])
    monkeypatch.setenv("GPX_BATCH_MAX", "64")
    np.testing.assert_array_equal(mlii.log_lh_batch(X, y, thetas, dtype=dtype), llh)


@pytest.mark.parametrize("N,d", [(16389, 5), (17408 + 63, 2)])
def test_ragged_sizes_above_16384(N, d):
    """n just above 16384: 512-wide outer block (the 1024-wide one starts above 32768 and has its own
    tests below), look-ahead on, CU-masked update stream off; the last block column is ragged (5 resp.
    63 columns).  Checked by size-independent properties."""
    X, y, Xo = orc.synth_inputs(N, d, 64)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s)
    alpha = g.inv_Kxx_y
    rows = np.array([0, 1, 1023, 1024, 8191, 16383, 16384, N - 2, N - 1])
    Krows = orc.kernel_matrix("gaussian", "K", X[rows], X, (h, w))
    Krows[np.arange(rows.size), rows] += s * s
    np.testing.assert_allclose(Krows @ alpha, y[rows], rtol=1e-9, atol=1e-10)
    L = g.Lxx
    np.testing.assert_allclose(L[rows] @ L.T, Krows, rtol=1e-11, atol=1e-12)
    logdet = 2 * np.log(np.diag(L)).sum()
    np.testing.assert_allclose(g.log_lh, -0.5 * y @ alpha - 0.5 * logdet - 0.5 * N * np.log(2 * np.pi), rtol=1e-12)
    np.testing.assert_allclose(g.mean(Xo)[:8], orc.kernel_matrix("gaussian", "K", Xo[:8], X, (h, w)) @ alpha,
                               rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("N,d", [(2049, 2), (4097, 3), (12289 + 70, 2)])
def test_sizes_at_the_outer_block_boundaries(N, d):
    """n just above 2048 / 4096 / 12288: the outer block switches 128 -> 256 -> 512, the CU-masked
    update stream is on below 12288 and off above, and every size leaves a ragged last block column.
    Checked by size-independent properties (K alpha = y on sampled rows, log_lh identity from L)."""
    X, y, Xo = orc.synth_inputs(N, d, 16)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s)
    alpha = g.inv_Kxx_y
    rows = np.unique(np.array([0, 1, 63, 64, 255, 256, 511, 512, 1023, 1024, 2047, 2048, N // 2, N - 2, N - 1]))
    Krows = orc.kernel_matrix("gaussian", "K", X[rows], X, (h, w))
    Krows[np.arange(rows.size), rows] += s * s
    np.testing.assert_allclose(Krows @ alpha, y[rows], rtol=1e-9, atol=1e-10)
    L = g.Lxx
    np.testing.assert_allclose(L[rows] @ L.T, Krows, rtol=1e-11, atol=1e-12)
    logdet = 2 * np.log(np.diag(L)).sum()
    np.testing.assert_allclose(g.log_lh, -0.5 * y @ alpha - 0.5 * logdet - 0.5 * N * np.log(2 * np.pi), rtol=1e-12)


def test_device_gradient_vs_oracle_and_finite_differences():
    # dloglh_dtheta computed on the device (K^-1 stays in HBM)
    N, d = 700, 3
    X, y, _ = orc.synth_inputs(N, d, 4)
    h, w, s = 0.9, 0.6 * np.sqrt(d), 0.7
    g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s)
    o = orc.OracleGP("gaussian", (h, w), X, y, s)
    grad = g.dloglh_dtheta
    np.testing.assert_allclose(grad, o.dloglh_dtheta, rtol=1e-7, atol=1e-9)
    # central finite differences of the device log_lh (the reference's own check, test_gp.py:75-97)
    eps = 1e-5
    fd = np.empty(3)
    for i in range(3):
        p0, p1 = g.params.copy(), g.params.copy()
        p0[i] -= eps; p1[i] += eps
        g0, g1 = g.copy(), g.copy()
        g0.params = p0; g1.params = p1
        fd[i] = (g1.log_lh - g0.log_lh) / (2 * eps)
    np.testing.assert_allclose(grad, fd, rtol=1e-5, atol=1e-6)
    # a size that takes the aligned MFMA route: X = L^-T built on the leading rows only, W = X X^T with
    # the k-loop of every tile row starting at its own row (both skip the structural zeros of X)
    N2, d2 = 1536, 2
    X2, y2, _ = orc.synth_inputs(N2, d2, 4)
    g2 = gp.GP(gp.GaussianKernel(1.1, 0.45 * np.sqrt(d2)), X2, y2, s=0.8)
    o2 = orc.OracleGP("gaussian", (1.1, 0.45 * np.sqrt(d2)), X2, y2, 0.8)
    np.testing.assert_allclose(g2.dloglh_dtheta, o2.dloglh_dtheta, rtol=1e-7, atol=1e-9)
    Ki = g2.inv_Kxx
    np.testing.assert_allclose(Ki, o2.inv_Kxx, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(Ki, Ki.T, rtol=0, atol=1e-12)
    # 1-D periodic
    x1 = np.sort(np.random.RandomState(3).uniform(-5, 5, 300))
    y1 = np.sin(x1)
    gpk = gp.GP(gp.PeriodicKernel(1.1, 0.8, 2.3), x1, y1, s=0.5)
    opk = orc.OracleGP("periodic", (1.1, 0.8, 2.3), x1, y1, 0.5)
    np.testing.assert_allclose(gpk.dloglh_dtheta, opk.dloglh_dtheta, rtol=1e-7, atol=1e-9)


# ----------------------------------------------- the routes the headline numbers come from --
def _device_diag(g):
    """diag(L) straight from the handle's HBM matrix (strided copy of n elements; L is not downloaded)."""
    st = g._fit_pd()
    lib = _lib.load()
    A, lda = ctypes.c_void_p(), ctypes.c_int64()
    _lib.check(lib.gpx_gp_device_ptrs(st.handle, ctypes.byref(A), ctypes.byref(lda), None, None, None, None))
    es = 8 if g._dtype == _lib.F64 else 4
    out = np.empty(g._n, dtype=np.float64 if es == 8 else np.float32)
    _lib.check(lib.gpx_memcpy2d_d2h(out.ctypes.data_as(ctypes.c_void_p), es, A, (lda.value + 1) * es, es,
                                    g._n, None))
    return out.astype(np.float64)


def _sampled_rows_check(g, X, y, h, w, s, rows, rtol, atol):
    alpha = g.inv_Kxx_y
    Krows = orc.kernel_matrix("gaussian", "K", X[rows], X, (h, w))
    Krows[np.arange(rows.size), rows] += s * s
    np.testing.assert_allclose(Krows @ alpha, y[rows], rtol=rtol, atol=atol)
    return alpha


def test_outer_block_1024_route_vs_oracle(monkeypatch):
    """The nb = 1024 outer block is what N = 65536 (BASELINE config 4, bench.py's workload) runs with;
    by default it is only selected above n = 32768.  GPX_POTRF_NB (read per call) forces it at a size the
    oracle factors in seconds: 4.6 block columns, ragged last one, look-ahead on."""
    monkeypatch.setenv("GPX_POTRF_NB", "1024")
    N, d = 4700, 3
    X, y, Xo = orc.synth_inputs(N, d, 64)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s)
    o = orc.OracleGP("gaussian", (h, w), X, y, s)
    np.testing.assert_allclose(g.log_lh, o.log_lh, rtol=1e-10)
    np.testing.assert_allclose(g.inv_Kxx_y, o.inv_Kxx_y, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(g.mean(Xo), o.mean(Xo), rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(g.Lxx, o.Lxx, rtol=1e-9, atol=1e-12)


def test_n_above_32768_default_route_properties():
    """N = 33000 > 32768: the DEFAULT block-size choice is nb = 1024 (the headline route), ragged last
    block column (232 columns).  Size-independent properties only, nothing n x n leaves the device:
    K alpha = y on sampled rows (oracle kernel rows), and the log_lh identity with logdet taken from
    a device-side strided fetch of diag(L)."""
    N, d = 33000, 2
    X, y, Xo = orc.synth_inputs(N, d, 32)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s)
    rows = np.unique(np.array([0, 1, 1023, 1024, 2047, 16383, 16384, 32767, 32768, 32999, N // 3, N - 2]))
    alpha = _sampled_rows_check(g, X, y, h, w, s, rows, 1e-9, 1e-10)
    dg = _device_diag(g)
    assert (dg > 0).all()
    logdet = 2 * np.log(dg).sum()
    np.testing.assert_allclose(g.log_lh, -0.5 * y @ alpha - 0.5 * logdet - 0.5 * N * np.log(2 * np.pi),
                               rtol=1e-12)
    np.testing.assert_allclose(g.mean(Xo)[:8], orc.kernel_matrix("gaussian", "K", Xo[:8], X, (h, w)) @ alpha,
                               rtol=1e-9, atol=1e-11)


# (config 3 at size: tests/test_gpu_configs.py::test_config3_exact_size_fp64_anchor_against_the_oracle_then_fp32)


class _PlainRBF(gp.kernels.Kernel):
    """A pure-Python plugin kernel (no native id): only `K` and `params`, as the abstract
    contract of gp/kernels/base.py:59-80 requires.  numpy on the host."""

    def __init__(self, h, ell):
        self.h, self.ell = float(h), float(ell)

    @property
    def params(self):
        return np.array([self.h, self.ell])

    @params.setter
    def params(self, val):
        self.h, self.ell = float(val[0]), float(val[1])

    def K(self, x1, x2, out=None):
        a = np.asarray(x1, dtype=np.float64).reshape(len(x1), -1)
        b = np.asarray(x2, dtype=np.float64).reshape(len(x2), -1)
        d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        return self.h ** 2 * np.exp(-0.5 * d2 / self.ell ** 2)


@pytest.mark.parametrize("dtype,N", [("float64", 700), ("float64", 1), ("float64", 65), ("float32", 700)])
def test_plugin_kernel_path_vs_numpy(dtype, N):
    """The reference's L3 -> L2 contract: GP only ever calls self.K(x1, x2)
    (gp/gp.py:264,524,548,572).  A kernel without a native id goes host K() -> gpx_gp_set_K ->
    device factor, and mean / cov through gpx_gp_mean_from_K / gpx_gp_cov_from_K (GEMM with N = 1,
    ldc = 1).  Checked against the same formulas in numpy / scipy."""
    rng = np.random.RandomState(11)
    d, m = 2, 37
    X = rng.uniform(-3, 3, (N, d)); y = np.sin(X.sum(1)) + 0.1 * rng.randn(N)
    Xo = rng.uniform(-3, 3, (m, d))
    k = _PlainRBF(1.3, 0.9)
    s = 0.6
    assert getattr(k, "_native_kernel", None) is None
    g = gp.GP(k, X, y, s=s, dtype=dtype)
    Kxx = k(X, X) + s * s * np.eye(N)
    L = scipy.linalg.cholesky(Kxx, lower=True)
    alpha = scipy.linalg.cho_solve((L, True), y)
    llh = -0.5 * y @ alpha - np.log(np.diag(L)).sum() - 0.5 * N * np.log(2 * np.pi)
    Kxox = k(Xo, X)
    mean = Kxox @ alpha
    cov = k(Xo, Xo) - Kxox @ scipy.linalg.cho_solve((L, True), Kxox.T)
    if dtype == "float64":
        np.testing.assert_allclose(g.log_lh, llh, rtol=1e-10)
        np.testing.assert_allclose(g.inv_Kxx_y, alpha, rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(g.Lxx, L, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(g.mean(Xo), mean, rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(g.cov(Xo), cov, rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(g.Kxx, Kxx, rtol=0, atol=0)
    else:
        np.testing.assert_allclose(g.log_lh, llh, rtol=1e-4)
        np.testing.assert_allclose(g.mean(Xo), mean, rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(g.cov(Xo), cov, rtol=1e-2, atol=5e-3)
    # a parameter change through the plugin's own setter refits (s large enough that logdet stays above
    # MIN = -705.6: below it the reference's clamp, gp_c.pyx:22-23, returns -inf -- and so does this path)
    g.params = np.array([1.1, 0.7, 0.9])
    k2 = _PlainRBF(1.1, 0.7)
    K2 = k2(X, X) + 0.81 * np.eye(N)
    L2 = scipy.linalg.cholesky(K2, lower=True)
    llh2 = -0.5 * y @ scipy.linalg.cho_solve((L2, True), y) - np.log(np.diag(L2)).sum() - 0.5 * N * np.log(2 * np.pi)
    np.testing.assert_allclose(g.log_lh, llh2, rtol=1e-10 if dtype == "float64" else 1e-4)
    if N == 700 and dtype == "float64":
        g.params = np.array([1.1, 0.7, 0.5])             # logdet = -741 < MIN: the clamp fires
        assert g.log_lh == -np.inf and g.lh == 0


def test_plugin_kernel_nonpd_raises_like_the_reference():
    class Rank1(_PlainRBF):
        def K(self, x1, x2, out=None):
            return np.outer(np.ones(len(x1)), np.ones(len(x2)))
    X = np.linspace(0, 1, 50); y = np.sin(X)
    g = gp.GP(Rank1(1, 1), X, y, s=0)
    with pytest.raises(np.linalg.LinAlgError):
        g.Lxx
    assert g.log_lh == -np.inf


@pytest.mark.parametrize("n,m,d", [(65, 129, 2), (200, 131, 7), (300, 64, 32)])
def test_gaussian_derivative_members_nd_vs_oracle(n, m, d):
    """kmat_kernel MODE 1 / 2 (dK_dw, d2K_*) at d > 1: the golden vectors are 1-D (the reference is),
    the oracle restates gaussian_c.pyx:51-164 with r^2 summed over the d inputs."""
    rng = np.random.RandomState(n * 3 + d)
    a = rng.uniform(-2, 2, (n, d)); b = rng.uniform(-2, 2, (m, d))
    k = gp.GaussianKernel(1.2, 0.6 * np.sqrt(d))
    prm = k.params
    np.testing.assert_allclose(k.jacobian(a, b), orc.jacobian("gaussian", a, b, prm), rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(k.hessian(a, b), orc.hessian("gaussian", a, b, prm), rtol=1e-10, atol=1e-14)
    for name in ("dK_dh", "dK_dw", "d2K_dhdh", "d2K_dhdw", "d2K_dwdh", "d2K_dwdw"):
        np.testing.assert_allclose(getattr(k, name)(a, b), orc.kernel_matrix("gaussian", name, a, b, prm),
                                   rtol=1e-10, atol=1e-14)


def test_two_handles_and_a_foreign_thread_use_the_handle_device():
    """A handle remembers its device and makes it current in every entry point: it can be driven from
    a host thread that never called gpx_set_device (HIP's current device is per thread), and two live
    handles do not disturb each other."""
    import threading
    X, y, Xo = orc.synth_inputs(1500, 3, 16)
    h, w = 1.0, 0.5 * np.sqrt(3)
    g1 = gp.GP(gp.GaussianKernel(h, w), X, y, s=1.0, device=0)
    g2 = gp.GP(gp.GaussianKernel(h, 2 * w), X, y, s=0.7, device=0)
    o1 = orc.OracleGP("gaussian", (h, w), X, y, 1.0)
    o2 = orc.OracleGP("gaussian", (h, 2 * w), X, y, 0.7)
    res = {}

    def work():
        res["llh2"] = g2.log_lh
        res["mean1"] = g1.mean(Xo)

    t = threading.Thread(target=work); t.start(); t.join()
    np.testing.assert_allclose(g1.log_lh, o1.log_lh, rtol=1e-10)
    np.testing.assert_allclose(res["llh2"], o2.log_lh, rtol=1e-10)
    np.testing.assert_allclose(res["mean1"], o1.mean(Xo), rtol=1e-8, atol=1e-11)


def test_bench_two_ranks_on_one_gpu_from_a_plain_invocation():
    """`python bench.py --gpus 2` as the driver calls it (no launcher environment): the script starts
    its own two ranks; here both share GPU 0 and gloo moves the panels (RCCL cannot put two ranks on
    one device).  One JSON line, n_gpus = 2, and the residual check inside bench passes."""
    import subprocess
    import sys
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(GPX_DIST_BACKEND="gloo", GPX_BENCH_SINGLE_DEVICE="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--problem-n", "2048",
                        "--problem-d", "4", "--problem-m", "64", "--steps", "1", "--warmup", "1"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and np.isfinite(out["log_lh"])
    X, y, _ = orc.synth_inputs(2048, 4, 64)
    o = orc.OracleGP("gaussian", (1.0, 0.5 * np.sqrt(4)), X, y, 1.0)
    np.testing.assert_allclose(out["log_lh"], o.log_lh, rtol=1e-10)


@pytest.mark.parametrize("kind,N,d", [("gaussian", 150, 3), ("gaussian", 700, 3), ("gaussian", 1536, 2),
                                      ("periodic", 130, 1), ("periodic", 600, 1)])
def test_device_second_derivative_stack_vs_oracle(kind, N, d):
    """dlh_dtheta, d2lh_dtheta2, dm_dtheta on the device (csrc/gpx_deriv.hip: K^-1 and
    the K^-1 dK_i products resident, traces / quadratic forms fused, only scalars return) against the
    oracle's restatement of gp_c.pyx:52-131 (dense numpy products).  lh underflows to 0 beyond a few
    hundred points (log_lh < MIN) and the reference's lh-scaled derivatives are then identically zero;
    at those sizes the same device pass is checked through the Hessian of log_lh (extension) against
    central differences of the device gradient (itself checked against the oracle), and dm_dtheta --
    which carries no lh factor -- against the oracle and the mean's finite differences
    (gp/tests/test_gp.py:146-174)."""
    if kind == "gaussian":
        X, y, Xo = orc.synth_inputs(N, d, 24)
        prm, s = (0.9, 0.6 * np.sqrt(d)), 1.1
        g = gp.GP(gp.GaussianKernel(*prm), X, y, s=s)
    else:
        X = np.sort(np.random.RandomState(3).uniform(-5, 5, N)); y = np.sin(X)
        Xo = np.linspace(-4, 4, 24)
        prm, s = (1.1, 0.8, 2.3), 0.9
        g = gp.GP(gp.PeriodicKernel(*prm), X, y, s=s)
    o = orc.OracleGP(kind, prm, X, y, s)
    npar = len(g.params)
    if N <= 150:
        assert g.lh > 0                               # the reference's quantities are non-trivial here
    if g.lh > 0:
        scale = np.abs(o.d2lh_dtheta2).max()
        np.testing.assert_allclose(g.dlh_dtheta, o.dlh_dtheta, rtol=1e-7, atol=1e-9 * np.abs(o.dlh_dtheta).max())
        np.testing.assert_allclose(g.d2lh_dtheta2, o.d2lh_dtheta2, rtol=1e-6, atol=1e-8 * scale)
        # d2lh = lh (H + g g^T) with H the Hessian of log_lh
        gr = g.dloglh_dtheta
        np.testing.assert_allclose(g.lh * (g.d2loglh_dtheta2 + np.outer(gr, gr)), o.d2lh_dtheta2,
                                   rtol=1e-6, atol=1e-8 * scale)
    else:
        assert not g.d2lh_dtheta2.any() and not o.d2lh_dtheta2.any()
    H = g.d2loglh_dtheta2
    np.testing.assert_allclose(H, H.T, rtol=1e-9, atol=1e-10 * np.abs(H).max())
    eps = 1e-5
    fdH = np.empty((npar, npar))
    for i in range(npar):
        p0, p1 = g.params.copy(), g.params.copy()
        p0[i] -= eps; p1[i] += eps
        g0, g1 = g.copy(), g.copy()
        g0.params = p0; g1.params = p1
        fdH[i] = (g1.dloglh_dtheta - g0.dloglh_dtheta) / (2 * eps)
    np.testing.assert_allclose(H, fdH, rtol=2e-5, atol=2e-6 * np.abs(H).max())
    dm = g.dm_dtheta(Xo)
    odm = o.dm_dtheta(Xo)
    np.testing.assert_allclose(dm, odm, rtol=1e-6, atol=1e-8 * np.abs(odm).max())
    eps = 1e-6
    for i in range(npar):
        p0, p1 = g.params.copy(), g.params.copy()
        p0[i] -= eps; p1[i] += eps
        g0, g1 = g.copy(), g.copy()
        g0.params = p0; g1.params = p1
        fd = (g1.mean(Xo) - g0.mean(Xo)) / (2 * eps)
        np.testing.assert_allclose(dm[i], fd, rtol=1e-4, atol=1e-6 * max(1.0, np.abs(fd).max()))


# ------------------------------------------------- persistence + out-of-core build --
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_save_load_fitted_roundtrip(tmp_path, dtype, monkeypatch):
    """gpx_gp_save / gpx_gp_load: the factor streams HBM -> file -> HBM in row blocks (block size forced
    small so that several blocks and a ragged last one occur); the restored GP serves log_lh, alpha, mean,
    cov and Lxx bit-identically WITHOUT refitting."""
    monkeypatch.setenv("GPX_IO_BLOCK_BYTES", str(300 * 1111 * 8))
    N, d, m = 1111, 3, 20
    X, y, Xo = orc.synth_inputs(N, d, m)
    g = gp.GP(gp.GaussianKernel(1.1, 0.9), X, y, s=0.8, dtype=dtype)
    ref = dict(llh=g.log_lh, alpha=g.inv_Kxx_y, mean=g.mean(Xo), cov=g.cov(Xo), L=g.Lxx)
    path = tmp_path / "fit.gpx"
    g.save_fitted(path)
    es = 8 if dtype == "float64" else 4
    assert os.path.getsize(path) < 0.8 * N * N * es + (N * (d + 2)) * 8 + 4096       # lower trapezoid, not n^2
    h = gp.GP.load_fitted(path)
    assert isinstance(h.K, gp.GaussianKernel) and np.array_equal(h.params, g.params)
    npdt = np.float64 if dtype == "float64" else np.float32        # x, y come back as the device holds them
    assert np.array_equal(h.x, g.x.astype(npdt).astype(np.float64)) and np.array_equal(h.y, g.y.astype(npdt).astype(np.float64))
    fit_version = h._dev.fit_version
    assert h.log_lh == ref["llh"]
    np.testing.assert_array_equal(h.inv_Kxx_y, ref["alpha"])
    np.testing.assert_array_equal(h.mean(Xo), ref["mean"])
    np.testing.assert_array_equal(h.cov(Xo), ref["cov"])
    np.testing.assert_array_equal(h.Lxx, ref["L"])
    assert h._dev.fit_version == fit_version                 # served from the loaded state
    h.s = 0.5                                                # and it is an ordinary GP afterwards
    o = orc.OracleGP("gaussian", (1.1, 0.9), X, y, 0.5)
    np.testing.assert_allclose(h.log_lh, o.log_lh, rtol=1e-10 if dtype == "float64" else 1e-4)
    with pytest.raises(ValueError):
        bad = tmp_path / "bad.gpx"
        bad.write_bytes(b"not a checkpoint")
        gp.GP.load_fitted(bad)


def test_extend_and_remove_adopt_the_fitted_handle():
    """The results of `extend` and `remove` carry a handle that is current (what `load_fitted` asserts above): reading
    `log_lh` does not refit."""
    n, d, k = 200, 2, 3
    X, y, _ = orc.synth_inputs(n + k, d, 1)
    g = gp.GP(gp.GaussianKernel(1.1, 0.9), X[:n], y[:n], s=0.8)
    for h, rows in ((g.extend(X[n:], y[n:]), n + k), (g.remove([0, 7, n - 1]), n - k)):
        assert h._dev.fit_version == h._version and h._dev.info == 0 and h.x.shape == (rows, d)
        assert h._dev.data_version == h._data_version and h._dev.params_version == h._version
        dev, fit_version = h._dev, h._dev.fit_version
        assert np.isfinite(h.log_lh)
        assert h._dev is dev and h._dev.fit_version == fit_version


def test_out_of_core_kernel_build_into_memmap(tmp_path, monkeypatch):
    """gpx_kmat_host streams row panels (panel size forced to 64 rows: 11 panels, ragged last) into the
    caller's buffer -- here a numpy.memmap, i.e. a matrix that never has to fit in HBM or host RAM."""
    monkeypatch.setenv("GPX_KMAT_PANEL_BYTES", "1")
    n, m, d = 700, 333, 5
    rng = np.random.RandomState(4)
    a = rng.uniform(-3, 3, (n, d)); b = rng.uniform(-3, 3, (m, d))
    k = gp.GaussianKernel(0.9, 1.7)
    out = np.memmap(tmp_path / "K.bin", dtype=np.float64, mode="w+", shape=(n, m))
    k(a, b, out=out)
    np.testing.assert_allclose(np.asarray(out), orc.kernel_matrix("gaussian", "K", a, b, k.params), rtol=1e-12, atol=1e-300)
    monkeypatch.delenv("GPX_KMAT_PANEL_BYTES")
    np.testing.assert_array_equal(k(a, b), np.asarray(out))            # one panel == many panels, bit for bit
    np.testing.assert_array_equal(k.dK_dw(a, b), _panelled(monkeypatch, lambda: k.dK_dw(a, b)))


def _panelled(monkeypatch, f):
    monkeypatch.setenv("GPX_KMAT_PANEL_BYTES", "1")
    try:
        return f()
    finally:
        monkeypatch.delenv("GPX_KMAT_PANEL_BYTES")


# ------------------------------------------------------- the C multi-GPU schedule (gpx_mg_*) --
@pytest.mark.parametrize("N,nb,force", [(2300, 256, False), (1500, 128, True), (4200, 1024, True)])
def test_native_mg_single_rank_rccl_vs_oracle(N, nb, force, monkeypatch):
    """gpx_mg_* with a ONE-rank RCCL communicator (librccl dlopen'ed, ncclCommInitRank with nranks = 1):
    the C schedule -- block-cyclic maps, look-ahead, pack kernel, chunked panel broadcast, distributed
    solves -- against the oracle; GPX_FORCE_COLLECTIVES makes every broadcast / all-reduce a real RCCL
    call on the handle's streams."""
    from gaussian_processes_amd import multi_gpu
    if force:
        monkeypatch.setenv("GPX_FORCE_COLLECTIVES", "1")
    d, m = 3, 40
    X, y, Xo = orc.synth_inputs(N, d, m)
    params = np.array([1.0, 0.5 * np.sqrt(d)])
    g = multi_gpu.NativeDistributedGP(N, d, nb=nb, backend="rccl", device=0)
    g.set_data(X, y)
    llh = g.fit(params, 1.0)
    o = orc.OracleGP("gaussian", params, X, y, 1.0)
    assert g.info == 0
    np.testing.assert_allclose(llh, o.log_lh, rtol=1e-10)
    np.testing.assert_allclose(g.alpha, o.inv_Kxx_y, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(g.mean(params, Xo), o.mean(Xo), rtol=1e-8, atol=1e-11)
    tm = g.timing()
    assert tm["factor"] > 0 and tm["chain_panel"] > 0 and tm["chain_update"] > 0
    # non-PD: info is the first failing minor, log_lh = -inf
    assert g.fit(np.array([1.0, 50.0]), 0.0) == -np.inf and g.info > 0
    g.close()


@pytest.mark.parametrize("world,N,nb,dtype_id", [(2, 3000, 256, 0), (3, 2500, 128, 0), (4, 5200, 512, 0), (2, 2100, 256, 1)])
def test_native_mg_world_on_one_gpu_vs_oracle(tmp_path, world, N, nb, dtype_id):
    """The same C schedule with `world` ranks sharing GPU 0, collectives through host callbacks over gloo
    (gpx_mg_create_cb): ownership maps, buffer reuse, chunked broadcasts and the distributed solves with
    real peers, against the oracle.  (4, 5200, 512): tall enough for the row-chunked broadcast path.)"""
    from _dist_helpers import run_native_world
    d, m = 3, 40
    res = run_native_world(world, N, d, nb, m, str(tmp_path), dtype_id=dtype_id)
    X, y, Xo = orc.synth_inputs(N, d, m)
    o = orc.OracleGP("gaussian", (1.0, 0.5 * np.sqrt(d)), X, y, 1.0)
    assert int(res["info"]) == 0
    if dtype_id == 0:
        np.testing.assert_allclose(float(res["log_lh"]), o.log_lh, rtol=1e-10)
        np.testing.assert_allclose(res["alpha"], o.inv_Kxx_y, rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(res["mean"], o.mean(Xo), rtol=1e-8, atol=1e-11)
    else:
        np.testing.assert_allclose(float(res["log_lh"]), o.log_lh, rtol=1e-4)
        np.testing.assert_allclose(res["mean"], o.mean(Xo), rtol=1e-3, atol=1e-3)
    assert float(res["log_lh2"]) == float(res["log_lh"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [1024, 2048, 2600, 3071, 5632])
def test_trsv_operator_form_vs_numpy(dtype, n, monkeypatch):
    """The operator form of the single-right-hand-side solves (W_k = inv(L_kk) by recursive doubling, Tf / Tb by
    batched 512^3 products, one launch per 512-block step), forced at small n by GPX_TRSV_OPS_MIN: exact
    multiples of 512, a ragged last block (40 / 511 columns), two and eleven full blocks; both directions
    against scipy, NaNs above the diagonal must never be read."""
    monkeypatch.setenv("GPX_TRSV_OPS_MIN", "1024")
    _lib.route_reset()
    npdt, did, tol = (np.float64, _lib.F64, 1e-11) if dtype == "f64" else (np.float32, _lib.F32, 3e-4)
    rng = np.random.RandomState(n)
    ld = ((n + 15) // 16) * 16
    Lh = rng.uniform(-1, 1, (n, ld)) / n ** 0.5
    Lh[:, n:] = np.nan
    for i in range(n):
        Lh[i, i] = 1.0 + rng.rand()
        Lh[i, i + 1:n] = np.nan
    y = rng.randn(n)
    lib = _lib.load()
    dL = DeviceBuffer.from_host(Lh.astype(npdt))
    tri = np.tril(Lh[:n, :n]).astype(npdt).astype(np.float64)
    z_ref = scipy.linalg.solve_triangular(tri, y.astype(npdt).astype(np.float64), lower=True)
    db = DeviceBuffer.from_host(y.astype(npdt))
    dz = DeviceBuffer((n,), npdt).zero()
    _lib.check(lib.gpx_d_trsv_lower(did, dL.ptr, n, ld, db.ptr, dz.ptr, 0, None))
    sync()
    z = dz.to_host().astype(np.float64)
    np.testing.assert_allclose(z, z_ref, rtol=tol, atol=tol * np.abs(z_ref).max())
    a_ref = scipy.linalg.solve_triangular(tri.T, z, lower=False)
    dzc = DeviceBuffer.from_host(dz.to_host())
    da = DeviceBuffer((n,), npdt).zero()
    _lib.check(lib.gpx_d_trsv_lower(did, dL.ptr, n, ld, dzc.ptr, da.ptr, 1, None))
    sync()
    np.testing.assert_allclose(da.to_host().astype(np.float64), a_ref, rtol=tol, atol=tol * np.abs(a_ref).max())
    # the route that was asked for is the route that ran (every switch is read per call): both sweeps in operator
    # form, none in the two-launch form -- and the other way round with the switch off
    assert _lib.route_count(_lib.ROUTE_TRSV_OPS) == 2 and _lib.route_count(_lib.ROUTE_TRSV_STEPS) == 0
    monkeypatch.setenv("GPX_TRSV_OPS", "0")
    _lib.route_reset()
    dzc = DeviceBuffer.from_host(dz.to_host())
    _lib.check(lib.gpx_d_trsv_lower(did, dL.ptr, n, ld, dzc.ptr, da.ptr, 1, None))
    sync()
    np.testing.assert_allclose(da.to_host().astype(np.float64), a_ref, rtol=tol, atol=tol * np.abs(a_ref).max())
    assert _lib.route_count(_lib.ROUTE_TRSV_OPS) == 0 and _lib.route_count(_lib.ROUTE_TRSV_STEPS) == 1


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N,ride,tail", [(3072, True, 4), (2560, True, 2), (4096, True, 4), (3072, False, 4), (1024, True, 1)])
def test_fit_builds_solve_operators_beside_the_factorisation(monkeypatch, dtype, N, ride, tail):
    """gpx_gp_fit (n a multiple of 512, by default from n = 8192): potrf() reports its progress, the block operators of
    the leading n / 512 - tail blocks are built on a stream of their own while the last panels are still being factored,
    and the backward sweep takes the trailing blocks by steps and the leading ones by their operators -- forced here at
    small n.  Against the route without it (bit-for-bit factor; alpha, log_lh, mean at the solve tolerance) and against
    the oracle; twice with one handle (the operator buffer is reused across factors), through the two-solve route
    (a forward sweep completes the set), and a later solve of the same factor (the gradient) completes it too."""
    d = 3
    X, y, Xo = orc.synth_inputs(N, d, 16)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 0.9
    o = orc.OracleGP("gaussian", (h, w), X, y, s)
    monkeypatch.setenv("GPX_FIT_OPS_AHEAD_MIN", "1024")
    monkeypatch.setenv("GPX_FIT_OPS_TAIL", str(tail))
    monkeypatch.setenv("GPX_TRSV_OPS_MIN", "1024")                 # later solves of the factor take the operator form: they complete the set
    if not ride:
        monkeypatch.setenv("GPX_FIT_RIDE_MAX", "0")
    out = {}
    for label, on in (("ahead", "1"), ("plain", "0")):
        monkeypatch.setenv("GPX_FIT_OPS_AHEAD", on)
        _lib.route_reset()
        g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s, dtype=dtype)
        first = (float(g.log_lh), np.array(g.inv_Kxx_y, dtype=np.float64), np.array(g.mean(Xo), dtype=np.float64),
                 np.array(g.Lxx, dtype=np.float64))
        assert (_lib.route_count(_lib.ROUTE_FIT_OPS_AHEAD) > 0) == (on == "1" and N // 512 > tail), (label, N, tail)
        grad = np.array(g.dloglh_dtheta, dtype=np.float64)       # later solves of the same factor
        g.set_param("w", 1.3 * w)                                  # a second factor with the same handle ...
        _ = float(g.log_lh)
        g.set_param("w", w)                                        # ... and back: must reproduce the first
        again = (float(g.log_lh), np.array(g.inv_Kxx_y, dtype=np.float64))
        out[label] = (first, grad, again)
    (lla, aa, ma, La), ga, (lla2, aa2) = out["ahead"]
    (llp, ap, mp, Lp), gp_, _ = out["plain"]
    assert np.array_equal(np.tril(La), np.tril(Lp))
    assert lla2 == lla and np.array_equal(aa2, aa)
    if dtype == "float64":
        np.testing.assert_allclose(aa, ap, rtol=1e-9, atol=1e-12 * np.abs(ap).max())
        np.testing.assert_allclose(lla, o.log_lh, rtol=1e-10)
        np.testing.assert_allclose(aa, o.inv_Kxx_y, rtol=1e-8, atol=1e-11 * np.abs(ap).max())
        np.testing.assert_allclose(ma, o.mean(Xo), rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(ga, o.dloglh_dtheta, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(ga, gp_, rtol=1e-9, atol=1e-11)
    else:
        np.testing.assert_allclose(aa, ap, rtol=2e-3, atol=2e-4 * np.abs(ap).max())
        np.testing.assert_allclose(lla, o.log_lh, rtol=1e-4)
        np.testing.assert_allclose(ma, o.mean(Xo), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N", [1024, 1536, 2048])
def test_cov_and_inverse_through_the_block_operators(monkeypatch, dtype, N):
    """X L^-T of the posterior covariance (gp/gp.py:599-625) and of inv_Kxx (:296-312) with n a multiple of 512: the
    substitution inside a 512-block is one product with inv(L_kk) from the factor's block operators (completed on
    demand) instead of eight 64-wide substitutions.  Against the 64-wide route (GPX_TRSM_OPS=0) and the oracle; the route
    counter says which one ran."""
    d = 2
    X, y, Xo = orc.synth_inputs(N, d, 37)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 0.9
    o = orc.OracleGP("gaussian", (h, w), X, y, s)
    out = {}
    for label, on in (("ops", "1"), ("steps", "0")):
        monkeypatch.setenv("GPX_TRSM_OPS", on)
        _lib.route_reset()
        g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s, dtype=dtype)
        out[label] = (np.array(g.cov(Xo), dtype=np.float64), np.array(g.inv_Kxx, dtype=np.float64),
                      np.array(g.dloglh_dtheta, dtype=np.float64))
        assert (_lib.route_count(_lib.ROUTE_TRSM_OPS) > 0) == (on == "1"), label
    if dtype == "float64":
        for label in out:
            np.testing.assert_allclose(out[label][0], o.cov(Xo), rtol=1e-7, atol=1e-10, err_msg=label)
            np.testing.assert_allclose(out[label][1], o.inv_Kxx, rtol=1e-7, atol=1e-9, err_msg=label)
            np.testing.assert_allclose(out[label][2], o.dloglh_dtheta, rtol=1e-7, atol=1e-9, err_msg=label)
        np.testing.assert_allclose(out["ops"][0], out["steps"][0], rtol=1e-10, atol=1e-12)
    else:
        for label in out:
            np.testing.assert_allclose(out[label][0], o.cov(Xo), rtol=1e-2, atol=5e-3, err_msg=label)
            np.testing.assert_allclose(out[label][2], o.dloglh_dtheta, rtol=2e-2, atol=1e-1, err_msg=label)


# ---- resident panel kernel (gpx_panel.hip): the default route of every panel of <= 256 columns ----

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N,nb", [(1990, "256"), (1990, "128"), (2048, "256"), (4171, "512"), (700, "256"), (64, "256"), (130, "128")])
def test_resident_panel_vs_launch_chain_and_oracle(monkeypatch, dtype, N, nb):
    """One launch per panel (rows in MFMA accumulators, leaf + inverse by the diagonal workgroup, sc1 hand-off of
    W = inv(L_jj) and of the diagonal rows' X blocks, left-looking pre-update by the columns to the left) against
    (a) the oracle and (b) the launch chain it replaces (GPX_POTRF_RES=0: leaf, substitution and update kernels),
    with the folded update on and off: ragged last workgroup, ragged last panel (old route), 1 - 4 steps,
    panels narrower than the matrix, a matrix smaller than one panel."""
    d = 3
    X, y, Xo = orc.synth_inputs(N, d, 16)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 0.9
    o = orc.OracleGP("gaussian", (h, w), X, y, s)
    monkeypatch.setenv("GPX_POTRF_NB", nb)
    res = {}
    for label, env in (("resident", {}), ("resident_nofold", {"GPX_POTRF_FOLD_ROWS": "0"}), ("chain", {"GPX_POTRF_RES": "0"})):
        for k in ("GPX_POTRF_FOLD_ROWS", "GPX_POTRF_RES"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _lib.route_reset()
        g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s, dtype=dtype)
        res[label] = (float(g.log_lh), np.array(g.Lxx, dtype=np.float64))
        n_res, n_chain = _lib.route_count(_lib.ROUTE_PANEL_RES), _lib.route_count(_lib.ROUTE_PANEL_CHAIN)
        if label == "chain":
            assert n_res == 0 and n_chain > 0, (label, n_res, n_chain)
        else:
            assert n_res > 0, (label, n_res, n_chain)            # (a ragged last panel still takes the chain)
    if dtype == "float64":
        for label, (llh, L) in res.items():
            np.testing.assert_allclose(llh, o.log_lh, rtol=1e-10, err_msg=label)
            np.testing.assert_allclose(np.tril(L), o.Lxx, rtol=1e-9, atol=1e-12, err_msg=label)
        np.testing.assert_allclose(np.tril(res["resident"][1]), np.tril(res["chain"][1]), rtol=1e-11, atol=1e-13)
    else:
        for label, (llh, L) in res.items():
            np.testing.assert_allclose(llh, o.log_lh, rtol=1e-4, err_msg=label)
            np.testing.assert_allclose(np.tril(L), o.Lxx, rtol=2e-3, atol=2e-4, err_msg=label)


@pytest.mark.parametrize("N", [700, 1990])
def test_fp32_resident_panel_both_leaf_forms_vs_oracle(monkeypatch, N):
    """The fp32 resident panel kernel exists in two instantiations: the leaf on the MFMA pipe (default for panels of up
    to 16384 rows and for the chain part of taller ones) and the lean one with the VALU sweep (GPX_LEAF_MFMA_F32_ROWS=0
    selects it everywhere).  Both against the oracle at the fp32 tolerances, and against each other."""
    d = 3
    X, y, Xo = orc.synth_inputs(N, d, 16)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 0.9
    o = orc.OracleGP("gaussian", (h, w), X, y, s)
    out = {}
    for label, rows in (("mfma", None), ("valu", "0")):
        if rows is None:
            monkeypatch.delenv("GPX_LEAF_MFMA_F32_ROWS", raising=False)
        else:
            monkeypatch.setenv("GPX_LEAF_MFMA_F32_ROWS", rows)
        g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s, dtype="float32")
        out[label] = (float(g.log_lh), np.array(g.Lxx, dtype=np.float64), np.array(g.mean(Xo), dtype=np.float64))
        np.testing.assert_allclose(out[label][0], o.log_lh, rtol=1e-4, err_msg=label)
        np.testing.assert_allclose(np.tril(out[label][1]), o.Lxx, rtol=2e-3, atol=2e-4, err_msg=label)
        np.testing.assert_allclose(out[label][2], o.mean(Xo), rtol=1e-3, atol=1e-3, err_msg=label)
    np.testing.assert_allclose(np.tril(out["mfma"][1]), np.tril(out["valu"][1]), rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_two_part_panel_launch_equals_one_launch(monkeypatch, dtype):
    """Tall panels (and lock-step batches with many rows in total) go out as two launches: the diagonal workgroups,
    then the rows, which then find every flag raised.  Forced here at sizes where one launch is the default
    (GPX_POTRF_TWO_PART_ROWS / _BATCH = 0): same arithmetic per workgroup, so the factor and log_lh must be equal bit
    for bit, single matrix and batch, and equal to the oracle's at the usual tolerance."""
    from gaussian_processes_amd import mlii
    N, d = 1990, 3
    X, y, _ = orc.synth_inputs(N, d, 4)
    thetas = np.array([[1.0, 0.9, 1.0], [0.7, 1.4, 0.8], [1.3, 0.6, 1.2]])
    ref = [orc.OracleGP("gaussian", th[:2], X, y, th[2]).log_lh for th in thetas]
    out = {}
    for label, env in (("one", {}), ("two", {"GPX_POTRF_TWO_PART_ROWS": "0", "GPX_POTRF_TWO_PART_BATCH": "0"})):
        for k in ("GPX_POTRF_TWO_PART_ROWS", "GPX_POTRF_TWO_PART_BATCH"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        g = gp.GP(gp.GaussianKernel(*thetas[0, :2]), X, y, s=thetas[0, 2], dtype=dtype)
        out[label] = (float(g.log_lh), np.array(g.Lxx), np.array(mlii.log_lh_batch(X, y, thetas, dtype=dtype)))
    assert out["one"][0] == out["two"][0]
    assert np.array_equal(np.tril(out["one"][1]), np.tril(out["two"][1]))
    assert np.array_equal(out["one"][2], out["two"][2])
    rtol = 1e-10 if dtype == "float64" else 1e-4
    np.testing.assert_allclose(out["two"][0], ref[0], rtol=rtol)
    np.testing.assert_allclose(out["two"][2], ref, rtol=rtol)


def test_resident_panel_reports_first_failing_minor():
    """A pivot <= 0 inside the resident kernel (diagonal workgroup 0, 1, 2 or 3 of a panel; first or later panel):
    info = LAPACK's first failing leading minor, nobody is left spinning, LinAlgError as the reference raises."""
    N = 1104                                               # (gpx_d_potrf wants lda % 16 == 0)
    rng = np.random.RandomState(3)
    B = rng.randn(N, N)
    A0 = B @ B.T + N * np.eye(N)
    lib = _lib.load()
    for bad in (0, 70, 130, 200, 255, 256, 300, 700, 1103):
        A = A0.copy()
        A[bad, bad] = -1.0                                 # minor bad + 1 is the first that is not positive definite
        dA = DeviceBuffer.from_host(A)
        info = DeviceBuffer((4,), np.int32).zero()
        _lib.check(lib.gpx_d_potrf(_lib.F64, dA.ptr, N, N, info.ptr, None))
        sync()
        assert int(info.to_host()[0]) == bad + 1, (bad, int(info.to_host()[0]))
        dA.free(); info.free()
    # fp32 (the MFMA leaf's float instantiation): the same convention
    for bad in (0, 70, 255, 700):
        A = A0.astype(np.float32)
        A[bad, bad] = -1.0
        dA = DeviceBuffer.from_host(A)
        info = DeviceBuffer((4,), np.int32).zero()
        _lib.check(lib.gpx_d_potrf(_lib.F32, dA.ptr, N, N, info.ptr, None))
        sync()
        assert int(info.to_host()[0]) == bad + 1, ("f32", bad, int(info.to_host()[0]))
        dA.free(); info.free()
    # and the same matrix without the defect still factors afterwards (flags / scratch left consistent)
    dA = DeviceBuffer.from_host(A0)
    info = DeviceBuffer((4,), np.int32).zero()
    _lib.check(lib.gpx_d_potrf(_lib.F64, dA.ptr, N, N, info.ptr, None))
    L = np.tril(dA.to_host())
    assert int(info.to_host()[0]) == 0
    np.testing.assert_allclose(L, scipy.linalg.cholesky(A0, lower=True), rtol=1e-10, atol=1e-12)


def test_resident_panel_interleaved_dtypes_and_batches(monkeypatch):
    """The published blocks live in a per-thread scratch whose layout must not depend on the call: fp64, fp32,
    a batch of 3, fp64 again, a batch of 2 in fp32 -- every result equal to the oracle's."""
    from gaussian_processes_amd import mlii
    N, d = 1350, 2
    X, y, _ = orc.synth_inputs(N, d, 4)
    thetas = np.array([[1.0, 0.9, 1.0], [0.7, 1.4, 0.8], [1.3, 0.6, 1.2]])
    ref = [orc.OracleGP("gaussian", th[:2], X, y, th[2]).log_lh for th in thetas]
    def single(dtype, i):
        g = gp.GP(gp.GaussianKernel(*thetas[i, :2]), X, y, s=thetas[i, 2], dtype=dtype)
        return float(g.log_lh)
    np.testing.assert_allclose(single("float64", 0), ref[0], rtol=1e-10)
    np.testing.assert_allclose(single("float32", 1), ref[1], rtol=1e-4)
    np.testing.assert_allclose(mlii.log_lh_batch(X, y, thetas, dtype="float64"), ref, rtol=1e-10)
    np.testing.assert_allclose(single("float64", 2), ref[2], rtol=1e-10)
    np.testing.assert_allclose(mlii.log_lh_batch(X, y, thetas[:2], dtype="float32"), ref[:2], rtol=1e-4)
    np.testing.assert_allclose(single("float32", 0), ref[0], rtol=1e-4)
    np.testing.assert_allclose(mlii.log_lh_batch(X, y, thetas, dtype="float64"), ref, rtol=1e-10)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N", [257, 1990, 4171])
def test_right_hand_side_riding_along_vs_two_solves(monkeypatch, dtype, N):
    """gpx_gp_fit / gpx_gp_fit_batch up to n = 16384: y is stored as row n of the matrix and takes part in every panel
    and update of the factorisation (potrf with one extra row), which leaves L^-1 y there -- the forward solve -- so
    only the backward solve runs.  Against the two-solve route (GPX_FIT_RIDE_MAX=0) and the oracle: alpha, log_lh, mean."""
    from gaussian_processes_amd import mlii
    d = 3
    X, y, Xo = orc.synth_inputs(N, d, 16)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 0.9
    o = orc.OracleGP("gaussian", (h, w), X, y, s)
    out = {}
    for label, env in (("ride", None), ("two_solves", "0")):
        if env is None:
            monkeypatch.delenv("GPX_FIT_RIDE_MAX", raising=False)
        else:
            monkeypatch.setenv("GPX_FIT_RIDE_MAX", env)
        _lib.route_reset()
        g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s, dtype=dtype)
        float(g.log_lh)
        assert _lib.route_count(_lib.ROUTE_FIT_RIDE if env is None else _lib.ROUTE_FIT_TWO_SOLVES) == 1
        assert _lib.route_count(_lib.ROUTE_FIT_TWO_SOLVES if env is None else _lib.ROUTE_FIT_RIDE) == 0
        out[label] = (float(g.log_lh), np.array(g.inv_Kxx_y, dtype=np.float64), np.array(g.mean(Xo), dtype=np.float64),
                      mlii.log_lh_batch(X, y, np.array([[h, w, s], [0.8, 1.1, 1.2]]), dtype=dtype))
    tol = dict(rtol=1e-9, atol=1e-11) if dtype == "float64" else dict(rtol=2e-3, atol=2e-4)
    for label, (llh, alpha, mean, batch) in out.items():
        np.testing.assert_allclose(llh, o.log_lh, rtol=1e-10 if dtype == "float64" else 1e-4, err_msg=label)
        np.testing.assert_allclose(alpha, o.inv_Kxx_y, err_msg=label, **tol)
        np.testing.assert_allclose(mean, o.mean(Xo), err_msg=label, **tol)
        np.testing.assert_allclose(batch[0], o.log_lh, rtol=1e-10 if dtype == "float64" else 1e-4, err_msg=label)
    np.testing.assert_allclose(out["ride"][1], out["two_solves"][1], **tol)
