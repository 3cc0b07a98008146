"""GPU tests of the chunked predictive variance: GP.var / GP.predict (gpx_gp_var, gpx_gp_var_from_K, gpx_d_var_rows) and
the distributed form (gpx_mg_var, NativeDistributedGP.var, DistributedGP.var / predict).

Tolerances are the project's own for the same quantity: the golden records' C_COND * cond(Kxx) * eps * scale bound of
tests/test_gpu_parity.py (restated below with the same constants), rtol 1e-7 / atol 1e-10 (fp32: 1e-2 / 5e-3) against the
oracle as for the diagonal of `cov` there, and 1e-10 * max|Kxoxo| between two device evaluations of the same quantity,
the bound of tests/test_gpu_dist_cov.py."""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib, multi_gpu
from oracle import gp_oracle as orc
from conftest import load_golden
from _dist_cov_helpers import ref_cov, run_ranks
from test_dist_gp_cpu import _PythonRBF

pytestmark = pytest.mark.gpu

C_COND = 16.0                      # tests/test_gpu_parity.py: |got - ref| <= C_COND * cond(Kxx) * eps * scale
_EPS = np.finfo(np.float64).eps
ORACLE_TOL = {"float64": dict(rtol=1e-7, atol=1e-10), "float32": dict(rtol=1e-2, atol=5e-3)}


def _records(npz, prefix):
    plen = len(prefix) + 2
    return {k[plen:]: npz[k] for k in npz.files if k.startswith(prefix + "__")}


GOLDEN_CASES = [("fixed", gp.GaussianKernel), ("periodic", gp.PeriodicKernel)] + \
    [("rand%02d" % i, gp.GaussianKernel) for i in range(16)] + [("prand%02d" % i, gp.PeriodicKernel) for i in range(6)]


def _record_bound(rec):
    """The `cov` line of tests/test_gpu_parity.py::_check_gp_record: tolerance and scale from the record itself."""
    tol = C_COND * float(np.linalg.cond(rec["Kxx"])) * _EPS
    rs = float(np.abs(rec["Kxox"]).sum(1).max())
    scale = np.abs(rec["Kxoxo"]).max() + rs * rs * np.abs(rec["inv_Kxx"]).max()
    return tol * max(float(scale), 1e-300)


def _check_var_record(g, rec):
    got, ref = g.var(rec["xo"]), np.diag(rec["cov"])
    err, bound = float(np.abs(got - ref).max()), _record_bound(rec)
    print("var vs golden: err %.3e bound %.3e" % (err, bound))
    assert got.shape == ref.shape
    assert err <= bound, "var: |got - ref| = %.3e exceeds C_COND cond eps scale = %.3e" % (err, bound)


@pytest.mark.parametrize("prefix,make_kernel", GOLDEN_CASES, ids=[c[0] for c in GOLDEN_CASES])
def test_var_golden_gp_small(prefix, make_kernel):
    rec = _records(load_golden("gp_small.npz"), prefix)
    kp, s = rec["params"][:-1], rec["params"][-1]
    _check_var_record(gp.GP(make_kernel(*kp), rec["x"], rec["y"], s=s), rec)


@pytest.mark.parametrize("n", [256, 1024])
def test_var_golden_gp_seeded_1d(n):
    g = _records(load_golden("gp_seeded_1d.npz"), "n%d" % n)
    m = gp.GP(gp.GaussianKernel(*g["params"][:2]), g["x"], g["y"], s=g["params"][2])
    np.testing.assert_allclose(m.var(g["xo"]), g["cov_diag"], rtol=1e-7, atol=1e-10)


# ---- against the oracle: both kernels, both dtypes, the operator route (N = 8192) and the 64-wide one ----
_ORACLE = {}
MS = [0, 1, 77, 700]


def _oracle_case(kind, N):
    """(X, y, Xo, kernel parameters, s, the oracle's diag cov at all 700 test points, the oracle), one CPU evaluation
    per (kind, N)."""
    if (kind, N) not in _ORACLE:
        d = 3 if kind == "gaussian" else 1
        X, y, Xo = orc.synth_inputs(N, d, max(MS))
        kp = (1.0, 0.5 * np.sqrt(d)) if kind == "gaussian" else (1.0, 0.8, 3.0)
        o = orc.OracleGP(kind, kp, X, y, 1.0)
        _ORACLE[(kind, N)] = (X, y, Xo, kp, 1.0, np.diag(o.cov(Xo)).copy(), o)
    return _ORACLE[(kind, N)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N", [1000, 4200, 8192])
@pytest.mark.parametrize("kind", ["gaussian", "periodic"])
def test_var_against_the_oracle(kind, N, dtype):
    X, y, Xo, kp, s, ref, _ = _oracle_case(kind, N)
    make = gp.GaussianKernel if kind == "gaussian" else gp.PeriodicKernel
    g = gp.GP(make(*kp), X.ravel() if X.shape[1] == 1 else X, y, s=s, dtype=dtype)
    g.log_lh                                                  # fit
    for m in MS:
        xo = Xo[:m].ravel() if X.shape[1] == 1 else Xo[:m]
        _lib.route_reset()
        got = g.var(xo)
        ops_var = _lib.route_count(_lib.ROUTE_TRSM_OPS)
        assert got.shape == (m,) and got.dtype == np.float64
        np.testing.assert_allclose(got, ref[:m], **ORACLE_TOL[dtype])
        assert _lib.route_count(_lib.ROUTE_VAR_CHUNK) == (1 if m else 0)
        if m:                                                 # the operator route where cov takes it, and only there
            _lib.route_reset()
            g.cov(xo)
            assert (ops_var > 0) == (_lib.route_count(_lib.ROUTE_TRSM_OPS) > 0)
            assert (ops_var > 0) == (N == 8192)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_var_plugin_kernel_through_var_from_K(dtype, monkeypatch):
    N, d = 1000, 3
    X, y, Xo = orc.synth_inputs(N, d, 700)
    h, ell, s = 1.3, 0.9, 1.0
    g = gp.GP(_PythonRBF(h, ell), X, y, s=s, dtype=dtype)
    K = _PythonRBF(h, ell)
    A = K.K(X, X) + s * s * np.eye(N)
    Kxox = K.K(Xo, X)
    ref = K.diag(Xo) - np.einsum("ij,ji->i", Kxox, np.linalg.solve(A, Kxox.T))
    for m in MS:
        got = g.var(Xo[:m])
        assert got.shape == (m,)
        np.testing.assert_allclose(got, ref[:m], **ORACLE_TOL[dtype])
    np.testing.assert_allclose(g.var(Xo), np.diag(g.cov(Xo)), **ORACLE_TOL[dtype])
    # the host evaluates Kxox in row chunks: forced to 100 rows a piece (and 128-row device chunks inside a piece of
    # 300), the same quantity within the bound between two device evaluations
    whole = g.var(Xo)
    for host_rows, chunk_rows in ((100, 0), (300, 128)):
        monkeypatch.setattr(gp.GP, "_VAR_HOST_CHUNK_BYTES", host_rows * N * 8)
        pieces = g.var(Xo, chunk_rows=chunk_rows)
        np.testing.assert_allclose(pieces, ref, **ORACLE_TOL[dtype])
        if dtype == "float64":
            assert np.abs(pieces - whole).max() <= 1e-10 * h * h


def _big():
    N, d = 8492, 3
    X, y, Xo = orc.synth_inputs(N, d, 1000)
    params = (1.0, 0.5 * np.sqrt(d))
    g = gp.GP(gp.GaussianKernel(*params), X, y, s=1.0)
    return g, X, y, Xo, params


def test_var_against_cov_on_the_same_object():
    g, X, y, Xo, params = _big()
    xo = Xo[:64]
    scale = float(np.abs(orc.kernel_matrix("gaussian", "K", xo, xo, params)).max())
    err = float(np.abs(g.var(xo) - np.diag(g.cov(xo))).max())
    print("var vs diag(cov): %.3e, bound %.3e" % (err, 1e-10 * scale))
    assert err <= 1e-10 * scale


def test_var_chunking_routes_repeatability_and_slices():
    g, X, y, Xo, params = _big()
    scale = float(np.abs(orc.kernel_matrix("gaussian", "K", Xo[:64], Xo[:64], params)).max())   # = k(x, x): the same at every point
    g.log_lh
    _lib.route_reset()
    auto = g.var(Xo)
    assert _lib.route_count(_lib.ROUTE_VAR_CHUNK) == 1 == _lib.var_plan(_lib.F64, X.shape[0], 1000)[1]
    _lib.route_reset()
    forced = g.var(Xo, chunk_rows=128)
    assert _lib.route_count(_lib.ROUTE_VAR_CHUNK) == 8 == _lib.var_plan(_lib.F64, X.shape[0], 1000, 128)[1]
    assert np.abs(forced - auto).max() <= 1e-10 * scale
    assert np.array_equal(g.var(Xo), auto)
    assert np.array_equal(g.var(Xo, chunk_rows=128), forced)
    assert np.array_equal(forced[128:256], g.var(Xo[128:256], chunk_rows=128))
    with pytest.raises(ValueError, match="chunk_rows"):
        g.var(Xo, chunk_rows=100)


def test_predict_and_noise():
    N, d = 1000, 3
    X, y, Xo = orc.synth_inputs(N, d, 77)
    g = gp.GP(gp.GaussianKernel(1.0, 0.5 * np.sqrt(d)), X, y, s=0.7)
    mean, var = g.predict(Xo)
    assert np.array_equal(mean, g.mean(Xo)) and np.array_equal(var, g.var(Xo))
    assert np.array_equal(g.var(Xo, noise=True), var + 0.7 ** 2)
    mean2, var2 = g.predict(Xo, noise=True)
    assert np.array_equal(mean2, mean) and np.array_equal(var2, var + 0.7 ** 2)


def test_var_at_two_hundred_thousand_points():
    """N = 8192, m = 200 000: the covariance would be 320 GB; the variance is 49 chunks of 4096 rows."""
    N, d, m = 8192, 3, 200000
    X, y, _, params, s, _, o = _oracle_case("gaussian", N)
    Xo = np.random.RandomState(7).uniform(-10, 10, (m, d))
    g = gp.GP(gp.GaussianKernel(*params), X, y, s=s)
    g.log_lh
    _lib.route_reset()
    var = g.var(Xo)
    assert _lib.route_count(_lib.ROUTE_VAR_CHUNK) == _lib.var_plan(_lib.F64, N, m)[1] >= 49
    kdiag = gp.GaussianKernel(*params).diag(Xo)
    assert var.shape == (m,) and np.isfinite(var).all()
    assert (var <= kdiag).all() and (var >= -1e-10 * kdiag).all()
    rows = np.sort(np.random.RandomState(11).choice(m, 64, replace=False))
    np.testing.assert_allclose(var[rows], np.diag(o.cov(Xo[rows])), rtol=1e-7, atol=1e-10)


def test_var_after_checkpoint_is_bit_identical(tmp_path):
    N, d = 1500, 3
    X, y, Xo = orc.synth_inputs(N, d, 300)
    g = gp.GP(gp.GaussianKernel(1.0, 0.5 * np.sqrt(d)), X, y, s=1.0)
    before = g.var(Xo, chunk_rows=128)
    path = str(tmp_path / "fit.gpx")
    g.save_fitted(path)
    h = gp.GP.load_fitted(path)
    assert np.array_equal(h.var(Xo, chunk_rows=128), before)
    assert np.array_equal(h.var(Xo), g.var(Xo))


def test_var_of_a_fit_that_is_not_positive_definite():
    rec = load_golden("gp_nonpd.npz")
    h, w, s = rec["params"]
    m = gp.GP(gp.GaussianKernel(h, w), rec["x"], rec["y"], s=s)
    errs = []
    for f in (m.cov, m.var, m.predict):
        with pytest.raises(np.linalg.LinAlgError) as e:
            f(rec["x"])
        errs.append(str(e.value))
    assert errs[0] == errs[1] == errs[2]


def test_d_var_rows_kernel_tails_alignment_and_kdiag():
    """gpx_d_var_rows alone: n that is no multiple of the vector width, an unaligned leading dimension, the caller's
    kdiag, the kernel family's diagonal (= the diagonal of gpx_d_kmat(xo, xo)), nothing read beyond n (the padding
    holds NaN), and the same bits twice."""
    lib = _lib.load()
    rng = np.random.RandomState(5)
    for dtype, npdt in ((_lib.F64, np.float64), (_lib.F32, np.float32)):
        es = np.dtype(npdt).itemsize
        for rows, n, ldx in ((5, 1, 16), (3, 1037, 1040), (7, 4099, 4112), (4, 333, 335), (2, 5000, 5008), (300, 64, 64)):
            d = 3
            Xh = np.full((rows, ldx), np.nan, dtype=npdt)
            Xh[:, :n] = rng.randn(rows, n)
            xo = rng.uniform(-3, 3, (rows, d)).astype(npdt)
            kd = rng.uniform(1, 2, rows)
            p = np.array([1.3, 0.7])
            bufs = [ctypes.c_void_p() for _ in range(5)]
            sizes = [Xh.nbytes, xo.nbytes, kd.nbytes, rows * 8, rows * rows * es]
            for b, sz in zip(bufs, sizes):
                _lib.check(lib.gpx_malloc(ctypes.byref(b), sz))
            try:
                dX, dxo, dkd, dout, dK = bufs
                for dst, src in ((dX, Xh), (dxo, xo), (dkd, kd)):
                    _lib.check(lib.gpx_memcpy_h2d(dst, src.ctypes.data_as(ctypes.c_void_p), src.nbytes, None))
                ss = (Xh[:, :n].astype(np.float64) ** 2).sum(1)
                out = np.empty(rows)
                _lib.check(lib.gpx_d_var_rows(dtype, _lib.KERNEL_GAUSSIAN, dX, rows, n, ldx, None, 0, None, dkd, dout, None))
                _lib.check(lib.gpx_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), dout, out.nbytes, None))
                np.testing.assert_allclose(out, kd - ss, rtol=1e-13, atol=1e-13 * ss.max())
                again = np.empty(rows)
                _lib.check(lib.gpx_d_var_rows(dtype, _lib.KERNEL_GAUSSIAN, dX, rows, n, ldx, None, 0, None, dkd, dout, None))
                _lib.check(lib.gpx_memcpy_d2h(again.ctypes.data_as(ctypes.c_void_p), dout, again.nbytes, None))
                assert np.array_equal(out, again)
                _lib.check(lib.gpx_d_kmat(dtype, _lib.KERNEL_GAUSSIAN, _lib.K, dxo, rows, dxo, rows, d, _lib.dptr(p), 0.0,
                                          _lib.FULL, dK, rows, None))
                Kh = np.empty((rows, rows), dtype=npdt)
                _lib.check(lib.gpx_memcpy_d2h(Kh.ctypes.data_as(ctypes.c_void_p), dK, Kh.nbytes, None))
                _lib.check(lib.gpx_d_var_rows(dtype, _lib.KERNEL_GAUSSIAN, dX, rows, 0, ldx, dxo, d, _lib.dptr(p), None, dout, None))
                _lib.check(lib.gpx_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), dout, out.nbytes, None))
                assert np.array_equal(out, np.diag(Kh).astype(np.float64))      # n = 0: kdiag itself
            finally:
                for b in bufs:
                    lib.gpx_free(b)


# ---- distributed ---------------------------------------------------------------------------------------------------
def _var_world(world, N, d, nb, calls, dtype_id=_lib.F64, kernel_id=_lib.KERNEL_GAUSSIAN, params=None, s=1.0):
    """Fit on `world` thread ranks, then var at the first m rows of Xo for every (m, chunk_rows) in calls."""
    X, y, Xo = orc.synth_inputs(N, d, max(m for m, _ in calls))
    params = np.array([1.0, 0.5 * np.sqrt(d)]) if params is None else params

    def body(rank, cb):
        g = multi_gpu.NativeDistributedGP(N, d, dtype_id=dtype_id, kernel_id=kernel_id, nb=nb, backend="callbacks",
                                          device=0, callbacks=cb)
        try:
            g.set_data(X, y)
            g.fit(params, s)
            assert g.info == 0
            return [g.var(params, Xo[:m], chunk_rows=c) for m, c in calls]
        finally:
            g.close()

    return X, y, Xo, params, run_ranks(world, body)


def test_rccl_world1_var_with_real_collectives(monkeypatch):
    monkeypatch.setenv("GPX_FORCE_COLLECTIVES", "1")
    N, d, m = 4200, 3, 200
    X, y, Xo = orc.synth_inputs(N, d, m)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    params = np.array([h, w])
    ref = np.diag(ref_cov("gaussian", (h, w), X, y, s, Xo)[0])
    g = multi_gpu.NativeDistributedGP(N, d, nb=1024, backend="rccl", device=0)
    try:
        assert g.comm_info()["rccl_nranks"] == 1
        g.set_data(X, y)
        g.fit(params, s)
        _lib.route_reset()
        var = g.var(params, Xo)
        assert _lib.route_count(_lib.ROUTE_TRSM_OPS) > 0 and _lib.route_count(_lib.ROUTE_VAR_CHUNK) == 1
        np.testing.assert_allclose(var, ref, rtol=1e-7, atol=1e-10)
        _lib.route_reset()
        np.testing.assert_allclose(g.var(params, Xo, chunk_rows=128), ref, rtol=1e-7, atol=1e-10)
        assert _lib.route_count(_lib.ROUTE_VAR_CHUNK) == 2
        assert np.abs(var - np.diag(g.cov(params, Xo))).max() <= 1e-10 * gp.GaussianKernel(h, w).diag(Xo[:1])[0]
    finally:
        g.close()


@pytest.mark.parametrize("world", [2, 8])
def test_thread_world_var_matches_single_gpu(world):
    N, d, nb, m = 8492, 3, 512, 64
    X, y, Xo, params, outs = _var_world(world, N, d, nb, [(m, 0)])
    v0 = outs[0][0]
    for r in range(1, world):
        assert np.array_equal(outs[r][0], v0), "rank %d differs from rank 0" % r
    single = gp.GP(gp.GaussianKernel(*params), X, y, s=1.0).var(Xo)
    scale = float(np.abs(orc.kernel_matrix("gaussian", "K", Xo, Xo, params)).max())
    err = float(np.abs(v0 - single).max())
    print("world %d vs single GPU: %.3e, bound %.3e" % (world, err, 1e-10 * scale))
    assert err <= 1e-10 * scale
    np.testing.assert_allclose(v0, np.diag(ref_cov("gaussian", tuple(params), X, y, 1.0, Xo)[0]), rtol=1e-7, atol=1e-10)


def test_world2_var_sizes_ragged_and_chunked():
    """m = 0, 1, 77, 700, automatic and 128-row chunks; 2100 = 8 x 256 + 52: a ragged last block, owned by rank 0."""
    N, d, nb = 2100, 3, 256
    calls = [(m, c) for m in MS for c in (0, 128)]
    X, y, Xo, params, outs = _var_world(2, N, d, nb, calls)
    ref = np.diag(ref_cov("gaussian", tuple(params), X, y, 1.0, Xo)[0])
    single = gp.GP(gp.GaussianKernel(*params), X, y, s=1.0).var(Xo)
    scale = float(np.abs(orc.kernel_matrix("gaussian", "K", Xo[:8], Xo[:8], params)).max())
    for i, (m, c) in enumerate(calls):
        assert outs[0][i].shape == (m,)
        assert np.array_equal(outs[0][i], outs[1][i])
        np.testing.assert_allclose(outs[0][i], ref[:m], rtol=1e-7, atol=1e-10)
        if m:
            assert np.abs(outs[0][i] - single[:m]).max() <= 1e-10 * scale


def test_world2_var_fp32():
    N, d, nb, m = 2100, 3, 256, 64
    X, y, Xo, params, outs = _var_world(2, N, d, nb, [(m, 0)], dtype_id=_lib.F32)
    ref = np.diag(ref_cov("gaussian", tuple(params), X, y, 1.0, Xo)[0])
    assert np.array_equal(outs[0][0], outs[1][0])
    np.testing.assert_allclose(outs[0][0], ref, rtol=1e-2, atol=5e-3)


def test_world2_var_periodic():
    N, d, nb, m = 2100, 1, 256, 64
    params = np.array([1.0, 0.8, 3.0])
    X, y, Xo, params, outs = _var_world(2, N, d, nb, [(m, 0)], kernel_id=_lib.KERNEL_PERIODIC, params=params)
    ref = np.diag(ref_cov("periodic", tuple(params), X, y, 1.0, Xo)[0])
    assert np.array_equal(outs[0][0], outs[1][0])
    np.testing.assert_allclose(outs[0][0], ref, rtol=1e-7, atol=1e-10)


def test_ranks_that_disagree_on_xo_or_chunk_rows_all_raise_and_the_handle_stays_usable():
    N, d, nb = 1000, 2, 128
    X, y, Xo = orc.synth_inputs(N, d, 300)
    params = np.array([1.0, 0.7])

    def body(rank, cb):
        g = multi_gpu.NativeDistributedGP(N, d, nb=nb, backend="callbacks", device=0, callbacks=cb)
        try:
            g.set_data(X, y)
            g.fit(params, 1.0)
            with pytest.raises(multi_gpu.RankMismatchError, match="gpx_mg_var.*different m"):
                g.var(params, Xo[:32 + rank])
            with pytest.raises(multi_gpu.RankMismatchError, match="gpx_mg_var.*different xo"):
                g.var(params, Xo[:32] + 0.5 * rank)
            with pytest.raises(multi_gpu.RankMismatchError, match="gpx_mg_var.*different chunk_rows"):
                g.var(params, Xo, chunk_rows=128 * rank)
            with pytest.raises(multi_gpu.RankMismatchError, match="gpx_mg_var.*multiple of 128"):
                g.var(params, Xo, chunk_rows=100 if rank else 0)
            return g.var(params, Xo, chunk_rows=128)
        finally:
            g.close()

    outs = run_ranks(2, body)
    assert np.array_equal(outs[0], outs[1])
    np.testing.assert_allclose(outs[1], np.diag(ref_cov("gaussian", tuple(params), X, y, 1.0, Xo)[0]), rtol=1e-7, atol=1e-10)


def test_distributed_gp_var_golden_records_world2():
    npz = load_golden("gp_small.npz")
    recs = [(_records(npz, p), k) for p, k in GOLDEN_CASES]

    def check_all(rank, cb):
        for rec, make_kernel in recs:
            kp, s = rec["params"][:-1], rec["params"][-1]
            g = gp.DistributedGP(make_kernel(*kp), rec["x"], rec["y"], s=s, backend="callbacks", callbacks=cb, device=0)
            try:
                _check_var_record(g, rec)
                mean, var = g.predict(rec["xo"])
                assert np.array_equal(mean, g.mean(rec["xo"])) and np.array_equal(var, g.var(rec["xo"]))
                assert np.array_equal(g.var(rec["xo"], noise=True), var + s ** 2)
            finally:
                g.close()
        return True

    assert run_ranks(2, check_all) == [True, True]


def test_distributed_gp_var_non_pd_on_every_rank():
    N, d = 600, 2
    X, y, Xo = orc.synth_inputs(N, d, 8)

    def body(rank, cb):
        g = gp.DistributedGP(gp.GaussianKernel(1.0, 0.7), X, y, s=1.0, backend="callbacks", callbacks=cb, nb=128, device=0)
        try:
            if rank == 1:
                _lib.check(_lib.load().gpx_debug_mg_inject_info(g.native.h, 5))
            assert g.log_lh == -np.inf
            for f in (lambda: g.var(Xo), lambda: g.predict(Xo)):
                with pytest.raises(np.linalg.LinAlgError):
                    f()
            # the C entry's own status, as gpx_mg_cov's
            out = np.empty(8)
            p = np.array([1.0, 0.7])
            rc = _lib.load().gpx_mg_var(g.native.h, _lib.dptr(p), _lib.dptr(np.ascontiguousarray(Xo)), 8, 0, _lib.dptr(out))
            assert rc == _lib.ERR_ARG and "not positive definite" in _lib.last_error()
            return g.native.info
        finally:
            g.close()

    assert run_ranks(2, body) == [5, 5]


def test_rehearsal_handle_has_no_var():
    lib = _lib.load()
    N, d = 1024, 2
    buf = ctypes.c_void_p()
    _lib.check(lib.gpx_malloc(ctypes.byref(buf), (N + 1) * N * 8 + N * 8))
    try:
        g = multi_gpu.NativeDistributedGP(N, d, nb=512, device=0, rehearsal=dict(
            rank=0, world=2, L_ptr=buf.value, ldl=N, alpha_ptr=buf.value + (N + 1) * N * 8))
        try:
            with pytest.raises(NotImplementedError, match="rehearsal"):
                g.var(np.array([1.0, 0.7]), np.zeros((4, d)))
            out, p, xo = np.empty(4), np.array([1.0, 0.7]), np.zeros((4, d))
            assert lib.gpx_mg_var(g.h, _lib.dptr(p), _lib.dptr(xo), 4, 0, _lib.dptr(out)) == _lib.ERR_UNSUPPORTED
        finally:
            g.close()
    finally:
        lib.gpx_free(buf)
