"""GPU tests of the distributed posterior covariance (gpx_mg_cov, NativeDistributedGP.cov) and of gp.DistributedGP: world 1
over a real RCCL communicator, thread worlds of 2 and 8 ranks on GPU 0, a two-process gloo world, fp32, the periodic
kernel, ragged blocks, m from 0 to beyond nb, the golden records, a non-PD fit, ranks that disagree, a rehearsal handle."""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib, multi_gpu
from oracle import gp_oracle as orc
from _dist_cov_helpers import check_record, ref_cov, run_gloo_world, run_ranks

pytestmark = pytest.mark.gpu


def _records(npz, prefix):
    plen = len(prefix) + 2
    return {k[plen:]: npz[k] for k in npz.files if k.startswith(prefix + "__")}


def _cov_world(world, N, d, nb, ms, dtype_id=_lib.F64, kernel_id=_lib.KERNEL_GAUSSIAN, params=None, s=1.0):
    """Fit on `world` thread ranks, then cov at the first m rows of Xo for every m in ms; every rank's results."""
    X, y, Xo = orc.synth_inputs(N, d, max(ms))
    params = np.array([1.0, 0.5 * np.sqrt(d)]) if params is None else params

    def body(rank, cb):
        g = multi_gpu.NativeDistributedGP(N, d, dtype_id=dtype_id, kernel_id=kernel_id, nb=nb, backend="callbacks",
                                          device=0, callbacks=cb)
        try:
            g.set_data(X, y)
            g.fit(params, s)
            assert g.info == 0
            return [g.cov(params, Xo[:m]) for m in ms]
        finally:
            g.close()

    return X, y, Xo, params, run_ranks(world, body)


def test_rccl_world1_cov_with_real_collectives(monkeypatch):
    """One RCCL rank, every all-reduce a real RCCL call; nb = 1024 (the diagonal blocks' operators from the fit: the
    operator route of the in-block solve), a ragged last block (4200 = 4 x 1024 + 104)."""
    monkeypatch.setenv("GPX_FORCE_COLLECTIVES", "1")
    N, d, m = 4200, 3, 200
    X, y, Xo = orc.synth_inputs(N, d, m)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    params = np.array([h, w])
    ref, ref_mean, _ = ref_cov("gaussian", (h, w), X, y, s, Xo)
    g = multi_gpu.NativeDistributedGP(N, d, nb=1024, backend="rccl", device=0)
    try:
        assert g.comm_info()["rccl_nranks"] == 1
        g.set_data(X, y)
        g.fit(params, s)
        _lib.route_reset()
        cov = g.cov(params, Xo)
        assert _lib.route_count(_lib.ROUTE_TRSM_OPS) > 0
        np.testing.assert_allclose(cov, ref, rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(g.mean(params, Xo), ref_mean, rtol=1e-8, atol=1e-11)
    finally:
        g.close()


@pytest.mark.parametrize("world", [2, 8])
def test_thread_world_cov_matches_single_gpu(world):
    N, d, nb, m = 8492, 3, 512, 64
    X, y, Xo, params, outs = _cov_world(world, N, d, nb, [m])
    c0 = outs[0][0]
    for r in range(1, world):
        assert np.array_equal(outs[r][0], c0), "rank %d differs from rank 0" % r
    single = gp.GP(gp.GaussianKernel(*params), X, y, s=1.0).cov(Xo)
    scale = float(np.abs(orc.kernel_matrix("gaussian", "K", Xo, Xo, params)).max())
    assert np.abs(c0 - single).max() <= 1e-10 * scale
    assert np.abs(c0 - c0.T).max() <= 1e-12 * scale
    assert (np.diag(c0) >= 0).all()


def test_world2_cov_sizes_ragged_and_beyond_nb():
    """m = 0, 1, 77 (not a multiple of 16) and 700 (> nb); 2100 = 8 x 256 + 52: a ragged last block, owned by rank 0."""
    N, d, nb = 2100, 3, 256
    ms = [0, 1, 77, 700]
    X, y, Xo, params, outs = _cov_world(2, N, d, nb, ms)
    ref, _, _ = ref_cov("gaussian", tuple(params), X, y, 1.0, Xo)
    for i, m in enumerate(ms):
        assert outs[0][i].shape == (m, m)
        assert np.array_equal(outs[0][i], outs[1][i])
        np.testing.assert_allclose(outs[0][i], ref[:m, :m], rtol=1e-7, atol=1e-10)


def test_world2_cov_fp32():
    N, d, nb, m = 2100, 3, 256, 64
    X, y, Xo, params, outs = _cov_world(2, N, d, nb, [m], dtype_id=_lib.F32)
    ref, _, _ = ref_cov("gaussian", tuple(params), X, y, 1.0, Xo)
    assert np.array_equal(outs[0][0], outs[1][0])
    np.testing.assert_allclose(outs[0][0], ref, rtol=1e-2, atol=5e-3)


def test_world2_cov_periodic():
    N, d, nb, m = 2100, 1, 256, 64
    params = np.array([1.0, 0.8, 3.0])
    X, y, Xo, params, outs = _cov_world(2, N, d, nb, [m], kernel_id=_lib.KERNEL_PERIODIC, params=params)
    ref, _, _ = ref_cov("periodic", tuple(params), X, y, 1.0, Xo)
    assert np.array_equal(outs[0][0], outs[1][0])
    np.testing.assert_allclose(outs[0][0], ref, rtol=1e-7, atol=1e-10)


def test_ranks_that_disagree_on_m_all_raise_and_the_handle_stays_usable():
    N, d, nb = 1000, 2, 128
    X, y, Xo = orc.synth_inputs(N, d, 40)
    params = np.array([1.0, 0.7])

    def body(rank, cb):
        g = multi_gpu.NativeDistributedGP(N, d, nb=nb, backend="callbacks", device=0, callbacks=cb)
        try:
            g.set_data(X, y)
            g.fit(params, 1.0)
            with pytest.raises(_lib.GpxError, match="different m"):
                g.cov(params, Xo[:32 + rank])
            with pytest.raises(_lib.GpxError, match="different xo"):
                g.cov(params, Xo[:32] + 0.5 * rank)
            return g.cov(params, Xo[:32])
        finally:
            g.close()

    outs = run_ranks(2, body)
    ref, _, _ = ref_cov("gaussian", tuple(params), X, y, 1.0, Xo[:32])
    np.testing.assert_allclose(outs[1], ref, rtol=1e-7, atol=1e-10)


def test_distributed_gp_gloo_two_processes(tmp_path):
    """gp.DistributedGP(dist=...) in two processes (host callbacks over gloo): log_lh, inv_Kxx_y, mean, cov against the
    oracle, and again after a change of params (the setter invalidates; the next member refits)."""
    res = run_gloo_world(2, str(tmp_path))
    N, d, m = 1500, 3, 50
    X, y, Xo = orc.synth_inputs(N, d, m)
    for kp, s, llh, cov in [((1.0, 0.5 * np.sqrt(d)), 1.0, "log_lh", "cov"), ((1.3, 0.7 * np.sqrt(d)), 0.8, "log_lh2", "cov2")]:
        o = orc.OracleGP("gaussian", kp, X, y, s)
        ref, ref_mean, ref_alpha = ref_cov("gaussian", kp, X, y, s, Xo)
        for r in res:
            assert int(r["world"]) == 2
            np.testing.assert_allclose(float(r[llh]), o.log_lh, rtol=1e-10)
            np.testing.assert_allclose(r[cov], ref, rtol=1e-7, atol=1e-10)
            if llh == "log_lh":
                np.testing.assert_allclose(r["alpha"], ref_alpha, rtol=1e-8, atol=1e-11)
                np.testing.assert_allclose(r["mean"], ref_mean, rtol=1e-8, atol=1e-11)


def test_distributed_gp_golden_records_world1_and_world2(golden):
    """gp_small's records (n = 16: one block column, which rank 1 does not own) through DistributedGP."""
    npz = golden("gp_small.npz")
    cases = [("fixed", gp.GaussianKernel), ("periodic", gp.PeriodicKernel)] + \
        [("rand%02d" % i, gp.GaussianKernel) for i in range(0, 16, 3)] + [("prand%02d" % i, gp.PeriodicKernel) for i in range(3)]
    recs = [(_records(npz, p), k) for p, k in cases]

    def check_all(callbacks):
        for rec, make_kernel in recs:
            kp, s = rec["params"][:-1], rec["params"][-1]
            g = gp.DistributedGP(make_kernel(*kp), rec["x"], rec["y"], s=s, backend="callbacks", callbacks=callbacks,
                                 device=0)
            try:
                check_record(g, rec)
            finally:
                g.close()
        return True

    assert check_all(None)                                        # world 1
    assert run_ranks(2, lambda rank, cb: check_all(cb)) == [True, True]


def test_distributed_gp_non_pd_on_every_rank():
    """A factor that is not positive definite on one rank (its info word set after the factorisation) is not positive
    definite on every rank: log_lh = -inf and lh = 0 everywhere, inv_Kxx_y / mean / cov raise LinAlgError everywhere."""
    N, d = 600, 2
    X, y, Xo = orc.synth_inputs(N, d, 8)

    def body(rank, cb):
        g = gp.DistributedGP(gp.GaussianKernel(1.0, 0.7), X, y, s=1.0, backend="callbacks", callbacks=cb, nb=128,
                             device=0)
        try:
            if rank == 1:
                _lib.check(_lib.load().gpx_debug_mg_inject_info(g.native.h, 5))
            assert g.log_lh == -np.inf and g.lh == 0
            for f in (lambda: g.inv_Kxx_y, lambda: g.mean(Xo), lambda: g.cov(Xo)):
                with pytest.raises(np.linalg.LinAlgError):
                    f()
            return g.native.info
        finally:
            g.close()

    assert run_ranks(2, body) == [5, 5]


def test_distributed_gp_rccl_new_shape_takes_over_the_communicator(monkeypatch):
    """World 1 over RCCL with real collectives: a change of n re-creates the handle on the same communicator."""
    monkeypatch.setenv("GPX_FORCE_COLLECTIVES", "1")
    X, y, Xo = orc.synth_inputs(700, 2, 30)
    kp, s = (1.0, 0.7), 1.0
    g = gp.DistributedGP(gp.GaussianKernel(*kp), X[:500], y[:500], s=s, device=0)
    try:
        first = g.native
        np.testing.assert_allclose(g.cov(Xo), ref_cov("gaussian", kp, X[:500], y[:500], s, Xo)[0], rtol=1e-7, atol=1e-10)
        g.x, g.y = X, y
        np.testing.assert_allclose(g.cov(Xo), ref_cov("gaussian", kp, X, y, s, Xo)[0], rtol=1e-7, atol=1e-10)
        assert g.native is not first and not first.h                  # the old handle is closed ...
        assert g.native.comm_info()["rccl_nranks"] == 1               # ... and its communicator lives on in the new one
    finally:
        g.close()


def test_rehearsal_handle_has_no_cov():
    lib = _lib.load()
    N, d = 1024, 2
    buf = ctypes.c_void_p()
    _lib.check(lib.gpx_malloc(ctypes.byref(buf), (N + 1) * N * 8 + N * 8))
    try:
        g = multi_gpu.NativeDistributedGP(N, d, nb=512, device=0, rehearsal=dict(
            rank=0, world=2, L_ptr=buf.value, ldl=N, alpha_ptr=buf.value + (N + 1) * N * 8))
        try:
            with pytest.raises(NotImplementedError, match="rehearsal"):
                g.cov(np.array([1.0, 0.7]), np.zeros((4, d)))
        finally:
            g.close()
    finally:
        lib.gpx_free(buf)
