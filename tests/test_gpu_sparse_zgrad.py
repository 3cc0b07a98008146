"""GPU tests of SparseGP's gradient in the inducing inputs (gpx_sgp_grad_z, csrc/gpx_sparse.hip; the rectangular pass
gpx_d_rect_zgrad of csrc/gpx_zgrad.hip) against the closed form of tests/_sparse_zgrad_helpers.py, which
tests/test_sparse_zgrad_cpu.py pins against central differences of the bound.

Tolerances of the parity test, per component (i, k).  fp64 (jitter 1e-6): ORACLE_TOL["float64"] (rtol 1e-7, atol 1e-10), or
C_COND cond(Kuu) eps scale_ik where that is larger: the rule of tests/test_gpu_sparse_grad.py with the helper's scale_ik (the
size of the terms that enter the component).  fp32: ORACLE_TOL["float32"] with the floor 4 rho scale_ik, rho = max_ik |fp32
restatement - fp64 restatement|_ik / scale_ik ONE number per key (the per-component difference is no floor for M d components:
tests/_sparse_zgrad_helpers.rho32); and, since that tolerance's atol of 5e-3 is the size of a whole component at these shapes,
rtol |ref| + floor without it as well (it held for every component of every key when this was written).  tests/test_sparse_zgrad_cpu.py asserts that the fp64 references stand 1e3 tolerances clear
and that the fp32 floor is below a tenth of the reference for 90 % of the components.  Every case prints error, bound and floor
of its worst component per dimension.

Shapes: (N, M) at the edges of the 64-tile and, with chunk_cols = 128, 2 and 3 ragged chunks, all three families; the Gaussian
family at 129 x 65 on both sides of every edge of the kernel's windows of dimensions (d = 4 | 5, 16 | 17, 32 | 33, 64 | 65); ARD at
d = 9, 17, 33.

The block alone (gpx_d_rect_zgrad) is compared with numpy in np.longdouble from the CAST inputs, the kernel values taken from
gpx_d_kmat on the same points: what is left is the block's own arithmetic.  Bound per component, in the convention of
tests/test_gpu_blocks.py:  4 (gamma_{n + 8} S + u |ref| + u_T S_k),  S = sum_j |coef_ji| k_ji |diff_jik| times the constants
(f64 products and sums of n terms; 8 more roundings for the coefficient, the constants, the divisor and the addition into out,
whose previous value is one more term), S_k the same sum with each term weighted by what a value of k formed in another order
may differ by: gaussian ((d + 2) |e_ji| + 4) roundings of T (e = -r^2 / 2 w^2: the squared distance's d + 1 roundings reach k
multiplied by |e|, then the product, the exponential and the constant); periodic (8 / w^2 + 8) |f| + 4 |arg| + 6 (sin of the
half angle arg within an ulp or two of the matrix build's, squared into the exponent -2 sin^2 / w^2; f = 2 sin cos from an
argument with two roundings)."""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from gaussian_processes_amd.device import DeviceBuffer, sync
from test_gpu_var import C_COND, ORACLE_TOL
from _block_helpers import DTYPES, LD, U, Worst, gamma, nan_in, nan_out, same_bits
from _sparse_helpers import CASES, S_NOISE, case_data
from _sparse_grad_helpers import EDGE_PAIRS
from _sparse_grad_helpers import make_kernel as case_kernel, problem as case_problem
from _sparse_zgrad_helpers import KEYS, KEY_IDS, key_jitter, make_kernel, problem, rho32, zgrad_reference

pytestmark = pytest.mark.gpu

_EPS = float(np.finfo(np.float64).eps)
START = np.array([1.5, 0.7, 1.3])


def _chunks(N, chunk_cols):
    return 1 if chunk_cols == 0 else -(-N // chunk_cols)          # automatic: every shape here fits one chunk


def _sparse(key, dtype="float64", chunk_cols=0):
    params, x, y, z = problem(key, dtype)
    auto = dtype == "float32" and key[0] != "periodic"
    sg = gp.SparseGP(make_kernel(key[0], params), x, y, S_NOISE, z, jitter=None if auto else key_jitter(key, dtype), dtype=dtype,
                     chunk_cols=chunk_cols)
    if auto:
        assert np.isclose(sg.jitter, key_jitter(key, dtype), rtol=1e-6, atol=0.0)
    return sg


def _assert_zgrad(key, dtype, got):
    ref, scale, cond = zgrad_reference(key, dtype)
    assert got.shape == ref.shape and got.dtype == np.float64
    tol = ORACLE_TOL[dtype]
    err = np.abs(got - ref)
    bound = tol["atol"] + tol["rtol"] * np.abs(ref)
    floor = C_COND * cond * _EPS * scale if dtype == "float64" else 4.0 * rho32(key) * scale
    ratio = (err / np.maximum(bound, floor)).reshape(ref.shape[0], -1)
    e2, b2, f2, r2 = (a.reshape(ref.shape[0], -1) for a in (err, bound, floor, ref))
    for k in range(ratio.shape[1]):
        i = int(np.argmax(ratio[:, k]))
        print("dz[%d, %d] %+.6e  err %.3e  bound %.3e  floor %.3e  (cond(Kuu) %.2e)%s"
              % (i, k, r2[i, k], e2[i, k], b2[i, k], f2[i, k], cond, "" if ratio[i, k] <= 1.0 else "  <-- FAILS"))
    print("%s %s: err <= rtol |ref| + floor (no atol) for %.1f %% of the components"
          % (key, dtype, 100.0 * np.mean(err <= tol["rtol"] * np.abs(ref) + floor)))
    assert np.isfinite(got).all()
    assert (ratio <= 1.0).all(), "components beyond tolerance: %d of %d, worst ratio %.3g" % ((ratio > 1.0).sum(), ratio.size, ratio.max())
    if dtype == "float32":
        # ORACLE_TOL's atol of 5e-3 is the size of a whole component here: the floor and the relative part alone hold as well
        assert (err <= tol["rtol"] * np.abs(ref) + floor).all()


@pytest.mark.parametrize("chunk_cols", [0, 128])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_parity_of_delbo_dz(key, dtype, chunk_cols):
    _lib.route_reset()
    sg = _sparse(key, dtype, chunk_cols)
    got = sg.delbo_dz
    assert _lib.route_count(_lib.ROUTE_SPARSE_CHUNK) == 2 * _chunks(key[1], chunk_cols)     # the fit's chunks, then ONE joint pass
    assert got.shape == sg.z.shape
    _assert_zgrad(key, dtype, got)


# ---- the block alone -----------------------------------------------------------------------------------------------------------
BLOCK_FAMILIES = [("gaussian", _lib.KERNEL_GAUSSIAN, 3), ("gaussian", _lib.KERNEL_GAUSSIAN, 5), ("gaussian", _lib.KERNEL_GAUSSIAN, 17),
                  ("periodic", _lib.KERNEL_PERIODIC, 1)]


def _block_params(family, d):
    return np.array([1.3, 0.9 * np.sqrt(d)]) if family == "gaussian" else np.array([1.1, 0.8, 2.3])


def _block_reference(family, params, r, q, K, C, u, v, scale, col_div, out0, u_T):
    """(ref, S, S_k) of the module docstring, np.longdouble, from the cast inputs and the device's own K (n x m)."""
    n, d = r.shape
    diff = (r[:, None, :] - q[None, :, :])                           # in T: the subtraction the kernel makes, r_jk - q_ik
    coef = C.astype(LD) + np.outer(u.astype(LD), v.astype(LD))
    g = coef * K.astype(LD)
    if family == "gaussian":
        w = LD(params[1])
        f, const = diff.astype(LD), 1 / (w * w)
        e = (diff.astype(LD) ** 2).sum(2) / (2 * w * w)
        weight = (((d + 2) * e + 4)[:, :, None]) * np.abs(f)
    else:
        w, p = LD(params[1]), LD(params[2])
        arg = diff.astype(LD) / (2 * p)
        f, const = np.sin(2 * arg), 1 / (p * w * w)
        weight = (8 / (w * w) + 8) * np.abs(f) + 4 * np.abs(arg) + 6
    const = const * LD(scale)
    div = np.ones(d, dtype=LD) if col_div is None else col_div.astype(LD)
    ref = out0.astype(LD) + const * (g[:, :, None] * f).sum(0) / div
    S = np.abs(out0).astype(LD) + np.abs(const) * (np.abs(g)[:, :, None] * np.abs(f)).sum(0) / div
    Sk = np.abs(const) * (np.abs(g)[:, :, None] * weight).sum(0) / div
    return ref, S + LD(u_T) * Sk / gamma(n + 8)           # (Worst.check multiplies its sum by gamma_{n + 8})


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_d_rect_zgrad(dtype):
    did, npdt, _, u_T = DTYPES[dtype]
    lib, rng, worst = _lib.load(), np.random.RandomState(211), Worst("gpx_d_rect_zgrad", dtype)
    for family, kid, d in BLOCK_FAMILIES:
        params = _block_params(family, d)
        for n, m in EDGE_PAIRS:
            r, q = rng.uniform(-3, 3, (n, d)).astype(npdt), rng.uniform(-3, 3, (m, d)).astype(npdt)
            dr, dq, dK = DeviceBuffer.from_host(r), DeviceBuffer.from_host(q), DeviceBuffer((n, m), npdt)
            _lib.check(lib.gpx_d_kmat(did, kid, _lib.K, dr.ptr, n, dq.ptr, m, d, _lib.dptr(params), 0.0, _lib.FULL, dK.ptr, m, None))
            sync()
            K = dK.to_host()
            need = ctypes.c_size_t(0)
            _lib.check(lib.gpx_rect_zgrad_scratch(kid, m, d, need))
            dpart = DeviceBuffer.from_host(np.full(need.value + 1, nan_out(np.float64)))
            # (C beyond its m columns is NaN: ldc > m) x (both parts, the outer product alone, C alone) x (plain, divisors)
            variants = [("both", 1.0, 1.0, 9, None, 1.0), ("C = 0", 0.0, 1.0, 0, None, -0.75), ("u = v = 0", 1.0, 0.0, 9, None, 2.5)]
            if family == "gaussian":
                variants.append(("col_div", 1.0, 1.0, 1, rng.uniform(0.5, 2.0, d), 1.0))
            for name, cs, us, pad, col_div, scale in variants:
                ldc = m + pad
                C = np.full((n, ldc), nan_in(npdt), dtype=npdt)
                C[:, :m] = cs * rng.randn(n, m)
                u, v = (us * rng.randn(n)).astype(npdt), (us * rng.randn(m)).astype(npdt)
                dC, du, dv = DeviceBuffer.from_host(C), DeviceBuffer.from_host(u), DeviceBuffer.from_host(v)
                out0 = np.full(m * d + 1, nan_out(np.float64))
                out0[:m * d] = rng.randn(m * d)
                got = []
                for _ in range(2):
                    dout = DeviceBuffer.from_host(out0)
                    _lib.check(lib.gpx_d_rect_zgrad(did, kid, dr.ptr, n, dq.ptr, m, d, _lib.dptr(params), dC.ptr, ldc, du.ptr, dv.ptr,
                                                    scale, None if col_div is None else _lib.dptr(col_div), dpart.ptr, dout.ptr, None))
                    sync()
                    got.append(dout.to_host())
                what = "%s d = %d n = %d m = %d %s" % (family, d, n, m, name)
                assert same_bits(got[0], got[1]), what + ": two runs differ"
                assert same_bits(got[0][m * d:], out0[m * d:]), what + ": wrote behind out"
                assert same_bits(dpart.to_host()[need.value:], np.full(1, nan_out(np.float64))), what + ": wrote behind the partials"
                ref, S = _block_reference(family, params, r, q, K, C[:, :m], u, v, scale, col_div, out0[:m * d].reshape(m, d), u_T)
                worst.check(got[0][:m * d].reshape(m, d), ref, S, n + 8, U, what)
    worst.report()


# ---- the joint call ------------------------------------------------------------------------------------------------------------
JOINT = [(("gaussian", 300, 3, 129), 128), (("ard", 129, 9, 65), 0), (("periodic", 300, 1, 129), 128), (("gaussian", 129, 17, 65), 128)]
JOINT_IDS = ["%s-%d-%d-%d-cols%d" % (k + (c,)) for k, c in JOINT]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("key,chunk_cols", JOINT, ids=JOINT_IDS)
def test_joint_call_gives_the_theta_gradient_bit_for_bit(key, chunk_cols, dtype):
    sg = _sparse(key, dtype, chunk_cols)
    st, lib = sg._fit_pd(), _lib.load()
    M, d, npar = sg.n_inducing, sg._d, sg.params.size
    alone = np.zeros(npar)
    _lib.check(lib.gpx_sgp_grad(st.handle, chunk_cols, _lib.dptr(alone)))
    _lib.route_reset()
    joint, gz = np.zeros(npar), np.zeros((M, d))
    _lib.check(lib.gpx_sgp_grad_z(st.handle, chunk_cols, _lib.dptr(joint), _lib.dptr(gz)))
    assert _lib.route_count(_lib.ROUTE_SPARSE_CHUNK) == _chunks(key[1], chunk_cols)          # one pass over x, not two
    assert same_bits(joint, alone)
    gz2 = np.zeros((M, d))
    _lib.check(lib.gpx_sgp_grad_z(st.handle, chunk_cols, None, _lib.dptr(gz2)))                # grad = NULL
    assert same_bits(gz2, gz) and np.any(gz != 0.0)
    assert lib.gpx_sgp_grad_z(st.handle, chunk_cols, _lib.dptr(joint), None) == _lib.ERR_ARG
    again = np.zeros(npar)
    _lib.check(lib.gpx_sgp_grad(st.handle, chunk_cols, _lib.dptr(again)))                      # ... and the theta-only pass after it
    assert same_bits(again, alone)
    # the Python side: delbo_dz leaves delbo_dtheta behind, served from the same call
    _lib.route_reset()
    assert same_bits(sg.delbo_dz, gz.reshape(sg.z.shape)) and same_bits(sg.delbo_dtheta, alone)
    assert _lib.route_count(_lib.ROUTE_SPARSE_CHUNK) == _chunks(key[1], chunk_cols)
    val, dth, dz = sg.elbo_and_grad(inducing=True)
    assert val == sg.elbo and same_bits(dth, alone) and same_bits(dz, sg.delbo_dz)
    assert _lib.route_count(_lib.ROUTE_SPARSE_CHUNK) == _chunks(key[1], chunk_cols)          # memoised
    t, tz = sg.grad_timing(), sg.zgrad_timing()
    assert set(tz) == {"kuu", "chunks"} and all(v >= 0 for v in tz.values())
    assert t["total"] >= max(t["mm"], t["build"], t["product"], t["reduce"], tz["chunks"])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case,chunk_cols", [(CASES[0], 128), (CASES[2], 0), (CASES[3], 128)], ids=["gaussian-128", "ard-auto", "periodic-128"])
def test_bits_repeat_and_the_fit_is_left_alone(case, chunk_cols, dtype):
    params, x, y, z0, xo, _ = case_data(case)
    z = z0 + 0.3 * np.random.RandomState(5).randn(*np.shape(z0))

    def fresh():
        return gp.SparseGP(case_kernel(case[0], params), x, y, S_NOISE, z, jitter=1e-6 if dtype == "float64" else None, dtype=dtype,
                           chunk_cols=chunk_cols)
    sg = fresh()
    before = dict(elbo=sg.elbo, mean=sg.mean(xo), var=sg.var(xo), Luu=sg.Luu.copy(), LB=sg.LB.copy(), c=sg.c.copy())
    dz = sg.delbo_dz
    assert np.isfinite(dz).all() and np.any(dz != 0.0)
    sg._memoized = {}
    assert sg.elbo == before["elbo"]
    assert np.array_equal(sg.mean(xo), before["mean"]) and np.array_equal(sg.var(xo), before["var"])
    for name in ("Luu", "LB", "c"):
        assert np.array_equal(getattr(sg, name), before[name]), name
    assert same_bits(sg.delbo_dz, dz)                                 # a second call on the same fit
    sg._memoized = {}
    sg.delbo_dtheta                                                   # ... and one after a theta-only gradient
    assert "grad_z" not in sg._memoized and same_bits(sg.delbo_dz, dz)
    assert same_bits(fresh().delbo_dz, dz)                            # a second object on the same data
    sg.s = 1.25                                                       # a setter invalidates it
    assert not np.array_equal(sg.delbo_dz, dz)


def test_failed_factorisation():
    case = CASES[4]
    _, x, y, z, _, _ = case_data(case)
    zz = np.array(z)
    zz[12:] = zz[:12]                                                # every inducing point twice, no jitter: Kuu has rank 12
    sg = gp.SparseGP(case_kernel(case[0], case_problem(case)[0]), x, y, S_NOISE, zz, jitter=0.0)
    st = sg._fit()
    assert st.stage == 1
    with pytest.raises(np.linalg.LinAlgError, match=r"stage 1 .*%d-th leading minor" % st.pivot):
        sg.delbo_dz
    val, grad, dz = sg.elbo_and_grad(inducing=True)
    assert val == -np.inf and grad.shape == (3,) and np.isnan(grad).all()
    assert dz.shape == zz.shape and dz.dtype == np.float64 and np.isnan(dz).all()
    grad_buf, z_buf = np.zeros(3), np.zeros(zz.size)
    assert _lib.load().gpx_sgp_grad_z(st.handle, 0, _lib.dptr(grad_buf), _lib.dptr(z_buf)) == _lib.ERR_ARG
    assert not z_buf.any()
    zt = ctypes.c_float * 2
    assert _lib.load().gpx_sgp_last_zgrad_timing(st.handle, zt()) == _lib.ERR_ARG


def _assert_timings(sg, joint):
    for t, stages in ((sg.fit_timing(), ("kuu", "build", "gram", "tail")), (sg.grad_timing(), ("mm", "build", "product", "reduce"))):
        assert set(t) == set(stages) | {"total"} and all(v >= 0 for v in t.values()), t
        assert t["total"] >= max(t[k] for k in stages), t
    if joint:
        tz = sg.zgrad_timing()
        assert set(tz) == {"kuu", "chunks"} and all(v >= 0 for v in tz.values()), tz
        assert sg.grad_timing()["total"] >= tz["chunks"]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_one_handle_through_alternating_passes_and_chunkings(dtype):
    """The handle's one pool of events grows (8 chunks), is reused at a smaller size (1 chunk) and grows no further; the work
    buffer is laid out anew by the fit and by the gradient in turn.  Nothing of that may show in a result."""
    case = CASES[0]
    assert case == ("gaussian", 1000, 3, 128)
    params, x, y, z, _, _ = case_data(case)

    def fresh(chunk_cols):
        return gp.SparseGP(case_kernel(case[0], params), x, y, S_NOISE, z, jitter=1e-6 if dtype == "float64" else None, dtype=dtype,
                           chunk_cols=chunk_cols)
    want8, want1 = fresh(128), fresh(0)
    sg = fresh(128)
    assert sg.elbo == want8.elbo and np.isfinite(sg.elbo)                              # 1. a fit in 8 chunks
    assert same_bits(sg.delbo_dz, want8.delbo_dz) and same_bits(sg.delbo_dtheta, want8.delbo_dtheta)      # 2.
    _assert_timings(sg, joint=True)
    sg.chunk_cols = 0                                                                  # 3. one chunk
    assert sg.elbo == want1.elbo and same_bits(sg.delbo_dtheta, want1.delbo_dtheta)    # 4.
    assert same_bits(sg.Luu, want1.Luu) and same_bits(sg.LB, want1.LB) and same_bits(sg.c, want1.c)
    _assert_timings(sg, joint=False)
    sg.chunk_cols = 128                                                                # 5.
    assert same_bits(sg.delbo_dz, want8.delbo_dz) and same_bits(sg.delbo_dtheta, want8.delbo_dtheta)      # 6.
    assert sg.elbo == want8.elbo and same_bits(sg.Luu, want8.Luu) and same_bits(sg.c, want8.c)
    _assert_timings(sg, joint=True)
    # a failed fit on the same handle: the rank-deficient z of test_failed_factorisation
    zz = np.array(z)
    zz[64:] = zz[:64]
    sg.jitter, sg.z = 0.0, zz
    st = sg._fit()
    assert st.stage == 1
    t = sg.fit_timing()
    assert t["total"] == t["kuu"] and t["kuu"] >= 0 and t["build"] == t["gram"] == t["tail"] == 0, t
    lib = _lib.load()
    assert lib.gpx_sgp_last_grad_timing(st.handle, (ctypes.c_float * 5)()) == _lib.ERR_ARG
    assert lib.gpx_sgp_last_zgrad_timing(st.handle, (ctypes.c_float * 2)()) == _lib.ERR_ARG


def test_joint_optimize_on_the_device():
    case = CASES[0]
    params, x, y, z, _, _ = case_data(case)
    z = z + 0.3 * np.random.RandomState(5).randn(*z.shape)
    sg = gp.SparseGP(case_kernel(case[0], params), x, y, S_NOISE, z, jitter=1e-6)
    sg.params = sg.params * START
    at_start = sg.elbo
    seen = []
    inner = sg.elbo_and_grad

    def spy(inducing=False):
        assert inducing
        out = inner(inducing=True)
        seen.append(out[0])
        return out
    sg.elbo_and_grad = spy
    _lib.route_reset()
    res = sg.optimize(maxiter=15, inducing=True)
    print("start %.6f -> %.6f in %d iterations, %d evaluations: %s" % (at_start, res["elbo"], res["nit"], res["nfev"], res["message"]))
    assert set(res) == {"params", "z", "elbo", "nit", "nfev", "success", "message"}
    assert len(seen) == res["nfev"]
    assert _lib.route_count(_lib.ROUTE_SPARSE_CHUNK) <= 2 * res["nfev"] + 1                  # a fit and ONE joint pass per evaluation
    assert res["elbo"] >= at_start
    assert res["elbo"] >= max(v for v in seen if np.isfinite(v))
    assert res["elbo"] > at_start                                    # it moved (the start is far from any optimum)
    assert np.array_equal(res["params"], sg.params) and np.array_equal(res["z"], sg.z) and res["z"].shape == z.shape
    assert not np.array_equal(res["z"], z)
    assert res["elbo"] == sg.elbo


def test_only_z_is_uploaded_when_only_z_moved(monkeypatch):
    key = ("gaussian", 129, 3, 65)
    sg = _sparse(key)
    real = _lib.load()
    calls = []

    class Spy(object):
        def __getattr__(self, name):
            return getattr(real, name)

        def gpx_sgp_set_data(self, handle, x, y, z):
            calls.append((x is not None, y is not None, z is not None))
            return real.gpx_sgp_set_data(handle, x, y, z)
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    first = sg.elbo
    assert calls == [(True, True, True)]
    z2 = np.array(sg.z) + 0.05
    sg.z = z2
    moved = sg.elbo
    assert calls[1:] == [(False, False, True)] and moved != first
    assert moved == gp.SparseGP(sg.K, sg.x, sg.y, S_NOISE, z2, jitter=sg.jitter).elbo         # the device holds x, y and the new z
    sg.params = sg.params * 1.1
    sg.elbo
    assert len(calls) == 3                                           # (the third: the fresh object's) parameters upload nothing
    sg.x = np.array(sg.x) + 0.01
    sg.elbo
    assert calls[3:] == [(True, True, True)]
