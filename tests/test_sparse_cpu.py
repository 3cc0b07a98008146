"""CPU tests of SparseGP: the numpy restatement of Titsias' bound that tests/test_gpu_sparse.py leans on is pinned against
the dense oracle (z = x, bound <= log_lh, monotone in M), the condition numbers under which the device is asked for the
project's fp64 tolerance are asserted, the fp32 error scale of every case is printed, SparseGP's refusals are checked with
the library call patched out, and the chunk / slice plan of a fit (host arithmetic) is pinned."""
from ctypes import POINTER, byref, c_double, c_int, c_int64, c_void_p
import re

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from oracle import gp_oracle as orc
from conftest import ROOT
from _sparse_helpers import (CASES, CASE_IDS, E32, JITTER64, PLAN_CASES, PLAN_IDS, QUANTITIES, S_NOISE, case_data, case_jitter,
                             kernel_params, oracle_view, plan_figures, reference, sgpr_reference)

c_double_p, c_int_p = POINTER(c_double), POINTER(c_int)


def _dense_oracle(case):
    params, x, y, _, xo, _ = case_data(case)
    okind, op, xv, xov = oracle_view(case[0], params, x, xo)
    return orc.OracleGP(okind, op, xv, y, S_NOISE), xov


def test_z_equal_x_is_the_dense_gp():
    """z = x, jitter 1.5e-8 on (1000, 3): the bound is the log marginal likelihood, the mean the dense mean, to the jitter's
    effect (measured: -1337.172196 against -1337.172192)."""
    X, y, Xo = orc.synth_inputs(1000, 3, 50)
    params = kernel_params("gaussian", 3)
    r = sgpr_reference("gaussian", params, X, y, X, 1.0, 1.5e-8)
    o = orc.OracleGP("gaussian", params, X, y, 1.0)
    print("bound %.6f  log_lh_chol %.6f" % (r["elbo"], o.log_lh_chol))
    assert abs(r["elbo"] - o.log_lh_chol) <= 1e-4
    err = np.abs(r["mean"](Xo) - o.mean(Xo)).max()
    print("mean: max |sparse - dense| = %.3e" % err)
    assert err <= 1e-4
    assert abs(sum(r["terms"].values()) - r["elbo"]) <= 1e-9 * abs(r["elbo"])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_bound_is_below_the_exact_log_lh(case):
    o, _ = _dense_oracle(case)
    r = reference(case, JITTER64)
    print("bound %.4f  log_lh %.4f" % (r["elbo"], o.log_lh_chol))
    assert r["elbo"] <= o.log_lh_chol + 1e-6


def test_bound_does_not_decrease_with_more_inducing_points():
    X, y, _ = orc.synth_inputs(1000, 3, 50)
    params = kernel_params("gaussian", 3)
    perm = np.random.RandomState(3).permutation(1000)
    bounds = [float(sgpr_reference("gaussian", params, X, y, X[perm[:M]], 1.0, JITTER64)["elbo"]) for M in (64, 128, 256)]
    print("bounds at M = 64, 128, 256:", bounds)
    assert bounds[0] <= bounds[1] <= bounds[2]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_condition_numbers_of_the_gpu_cases(case, dtype):
    """error ~ cond * eps: at cond(Kuu) <= 2e7 and cond(B) <= 100 the fp64 rtol of 1e-7 can be demanded of the device; the
    atol that goes with it needs the absolute figure below as well."""
    r = reference(case, case_jitter(case, dtype))
    cu, cb = np.linalg.cond(r["Kuu"]), np.linalg.cond(np.tril(r["B"]) + np.tril(r["B"], -1).T)
    print("%s jitter %.3e: cond(Kuu + eps I) %.3e  cond(B) %.3e" % (CASE_IDS[CASES.index(case)], case_jitter(case, dtype), cu, cb))
    assert cu <= 2e7
    assert cb <= 100
    # what either implementation can know of an entry of X = B - I (and so of LB, c): cond(Kuu) eps max|X|, absolute.  The
    # GPU tests ask for atol = 1e-10 elementwise in fp64, entries near zero included (fp32 has its own floor, E32)
    X = r["B"] - np.eye(case[3])
    amp = cu * np.finfo(dtype).eps * np.abs(X).max()
    print("    cond(Kuu) eps max|X| = %.3e" % amp)
    if dtype == np.float64:
        assert amp <= 1e-10


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_fp32_error_scale(case):
    """The float32 run of the restatement against the float64 run, per quantity: finite, and printed for the record."""
    e = E32[case]
    print(CASE_IDS[CASES.index(case)], " ".join("%s %.2e" % (k, e[k]) for k in QUANTITIES))
    assert set(e) == set(QUANTITIES)
    assert all(np.isfinite(v) for v in e.values())


def test_subset_inducing_is_a_pure_function():
    x = np.arange(40.0).reshape(20, 2)
    a, b = gp.SparseGP.subset_inducing(x, 7, seed=3), gp.SparseGP.subset_inducing(x, 7, seed=3)
    assert np.array_equal(a, b) and a.shape == (7, 2)
    assert len({tuple(r) for r in a}) == 7 and all(tuple(r) in {tuple(q) for q in x} for r in a)
    assert np.array_equal(a, x[np.random.RandomState(3).permutation(20)[:7]])
    assert not np.array_equal(a, gp.SparseGP.subset_inducing(x, 7, seed=4))
    for M in (0, 21):
        with pytest.raises(ValueError):
            gp.SparseGP.subset_inducing(x, M)


def test_sparse_symbols_are_bound():
    want = {
        "gpx_sgp_create": (c_int, [POINTER(c_void_p), c_int, c_int, c_int64, c_int64, c_int]),
        "gpx_sgp_fit": (c_int, [c_void_p, c_double_p, c_double, c_double, c_int64, c_int_p, c_int_p]),
        "gpx_sgp_var": (c_int, [c_void_p, c_double_p, c_int64, c_int64, c_double_p]),
        "gpx_sgp_get": (c_int, [c_void_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    }
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name][0] is res
        assert list(_lib._SIGNATURES[name][1]) == args, name
    assert (_lib.ROUTE_SPARSE_CHUNK, _lib.PROF_SPARSE_GRAM) == (25, 19)
    with open(ROOT + "/include/gpx.h") as f:
        hdr = f.read()
    for macro, value in (("GPX_ROUTE_SPARSE_CHUNK", 25), ("GPX_PROF_SPARSE_GRAM", 19)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), hdr)
    assert not hasattr(gp.SparseGP, "log_lh")


# ---- refusals come before the library is touched ----
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def _data(d=3, n=10, M=4):
    rng = np.random.RandomState(0)
    x = rng.randn(n, d) if d > 1 else rng.randn(n)
    return x, rng.randn(n), x[:M].copy()


def _make(**kw):
    x, y, z = _data()
    args = dict(K=gp.GaussianKernel(1.0, 1.0), x=x, y=y, s=1.0, z=z)
    args.update(kw)
    return gp.SparseGP(**args)


@pytest.mark.parametrize("kw", [
    dict(s=0.0), dict(s=-1.0), dict(s=np.nan),
    dict(jitter=-1e-6), dict(jitter=np.inf), dict(jitter=np.nan),
    dict(z=np.zeros((4, 2))), dict(z=np.zeros(4)), dict(z=np.zeros((0, 3))), dict(z=np.zeros((2, 3, 1))),
    dict(chunk_cols=-128), dict(chunk_cols=100),
], ids=["s0", "s_neg", "s_nan", "jitter_neg", "jitter_inf", "jitter_nan", "z_wrong_d", "z_1d", "M0", "z_3d", "chunk_neg", "chunk_100"])
def test_constructor_refusals(no_library, kw):
    with pytest.raises(ValueError):
        _make(**kw)


def test_plugin_kernel_is_refused(no_library):
    class Plugin(gp.Kernel):
        pass
    x, y, z = _data()
    with pytest.raises(NotImplementedError):
        gp.SparseGP(Plugin.__new__(Plugin), x, y, 1.0, z)


def test_prediction_refusals(no_library):
    sg = _make()
    for call in (sg.mean, sg.var, sg.cov, sg.predict):
        for xo in (np.zeros((5, 2)), np.zeros(5), np.zeros((5, 3, 1))):
            with pytest.raises(ValueError):
                call(xo)
    for chunk_rows in (-128, 64, 200):
        with pytest.raises(ValueError):
            sg.var(np.zeros((5, 3)), chunk_rows=chunk_rows)
    for name, val in (("s", 0.0), ("jitter", -1.0), ("chunk_cols", 64), ("z", np.zeros((3, 2)))):
        with pytest.raises(ValueError):
            setattr(sg, name, val)


def test_setters_invalidate(no_library):
    sg = _make()
    v, dv = sg._version, sg._data_version
    sg.s = 1.0                                   # nothing changes: nothing is invalidated
    sg.z = sg.z.copy()
    sg.params = sg.params.copy()
    assert (sg._version, sg._data_version) == (v, dv)
    sg.s = 2.0
    assert sg._version == v + 1 and sg._data_version == dv
    sg.z = sg.x[2:7]
    assert sg._data_version == dv + 1 and sg.n_inducing == 5
    p = sg.params
    p[1] *= 2
    sg.params = p
    assert sg.K.params[1] == p[1] and sg._version > v + 2
    assert sg.jitter == np.sqrt(np.finfo(np.float64).eps) * sg.K.diag(sg.z[:1])[0]
    assert gp.SparseGP(gp.GaussianKernel(1.0, 1.0), *_data()[:2], 1.0, _data()[2], dtype="float32").jitter == \
        np.sqrt(np.finfo(np.float32).eps) * sg.K.__class__(1.0, 1.0).diag(sg.z[:1])[0]


# ---- the plan of a fit: host arithmetic (no GPU) ----
def _plan(n, M, chunk_cols=0, split=0, free=1 << 36, dtype=_lib.F64):
    cols, chunks, slices, width = c_int64(0), c_int64(0), c_int(0), c_int64(0)
    _lib.check(_lib.load().gpx_debug_sgp_plan(dtype, n, M, chunk_cols, split, free, byref(cols), byref(chunks), byref(slices),
                                              byref(width)))
    return cols.value, chunks.value, slices.value, width.value


def test_plan_of_a_fit():
    assert _plan(1000, 128, 128) == (128, 8, 1, 128)               # the tests' explicit chunks: 7 whole ones and 104 columns
    assert _plan(777, 64, 128)[:2] == (128, 7) and _plan(300, 300, 128)[:2] == (128, 3)
    # automatic: one chunk no wider than the data; 16 slices planned, none narrower than 128 columns
    assert _plan(1000, 128) == (1024, 1, 8, 128)
    assert _plan(2000, 256) == (2048, 1, 16, 128)
    for M in (1024, 2048, 4096):
        assert _plan(1 << 20, M) == (16384, 64, 8, 2048)           # the measured shapes of DESIGN 3.3
    assert _plan(1 << 20, 128) == (16384, 64, 16, 1024)            # one tile: as many slices as the cap allows
    assert _plan(1 << 20, 4096, split=1) == (16384, 64, 1, 16384)
    assert _plan(1 << 20, 1024, split=4) == (16384, 64, 4, 4096)
    assert _plan(1 << 22, 16384)[2] == 1                           # accumulators of 2 GiB each: one
    assert _plan(1 << 22, 16384, dtype=_lib.F32)[2] == 2
    assert _plan(1 << 20, 1024, free=1 << 30) == (16384, 64, 8, 2048)
    assert _plan(1 << 20, 4096, free=1 << 30)[0] == 8192           # a quarter of 1 GiB holds 8192 columns of 4096 rows
    for bad in (-128, 100):
        with pytest.raises(ValueError):
            _plan(1000, 128, bad)
    with pytest.raises(MemoryError):
        _plan(1000, 4096, free=1 << 20)
    with pytest.raises(MemoryError):
        _plan(1 << 20, 4096, 16384, free=1 << 30)


@pytest.mark.parametrize("dtype", [_lib.F64, _lib.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case,plan,figures", PLAN_CASES, ids=PLAN_IDS)
def test_depth_slice_plans_of_the_gpu_tests(case, plan, figures, dtype):
    """The plans tests/test_gpu_sparse.py fits with are what tests/_sparse_helpers.py says they are, in both dtypes."""
    _, N, _, M = case
    assert plan_figures(_plan(N, M, plan[0], plan[1], dtype=dtype), N) == figures
    assert _plan(N, M, dtype=dtype)[1] == 1                        # the plan they are compared with: one chunk
