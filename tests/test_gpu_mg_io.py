"""GPU tests of the distributed handle's host <-> device transfers (csrc/gpx_mg.hip goes through the single-GPU handle's
upload_f64 / download_f64): an fp32 handle rounds the caller's float64 on the DEVICE, and that has to be the rounding
numpy does on the host -- IEEE round to nearest, ties to even, subnormals included -- bit for bit; and the staging copy
those uploads need is allocated before the ranks of a collective prediction agree, so a refused call leaves nothing
behind.  Also the smallest distributed fit that takes the trailing update's generic route past a ragged last block column
(three thread-ranks, nb = 64, N = 209)."""
import ctypes

import numpy as np
import pytest

from gaussian_processes_amd import _lib, multi_gpu
from oracle import gp_oracle as orc
from _dist_cov_helpers import ref_cov, run_ranks

pytestmark = pytest.mark.gpu

# float64 values that are no float32 numbers: a tie that rounds to even (1.0), one that rounds up, a tie among the fp32
# subnormals (1.5 * 2**-149 -> 2**-148), the first one negated
AWKWARD = np.array([1 + 2.0 ** -24, 1 + 3 * 2.0 ** -25, 3 * 2.0 ** -150, -(1 + 2.0 ** -24)])


def _through_f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def test_awkward_values_are_what_they_claim():
    want = np.array([1.0, 1 + 2.0 ** -23, 2.0 ** -148, -1.0])
    assert np.array_equal(_through_f32(AWKWARD), want) and not np.array_equal(AWKWARD, want)


def test_fp32_upload_rounds_on_the_device_as_numpy_does_on_the_host():
    lib = _lib.load()
    n, d = 8, 1
    x = np.concatenate([AWKWARD, [0.1, -2.7, 1e10 / 3, 123.456]]).reshape(n, d)
    y = np.ascontiguousarray(x[::-1, 0] * (1 + 2.0 ** -30))
    h = ctypes.c_void_p()
    _lib.check(lib.gpx_gp_create(ctypes.byref(h), _lib.F32, _lib.KERNEL_GAUSSIAN, n, d))
    try:
        _lib.check(lib.gpx_gp_set_data(h, _lib.dptr(x), _lib.dptr(y)))
        gx, gy = np.empty((n, d)), np.empty(n)
        _lib.check(lib.gpx_gp_get_xy(h, _lib.dptr(gx), _lib.dptr(gy)))
    finally:
        lib.gpx_gp_destroy(h)
    print("x back:", [v.hex() for v in gx.ravel()], "\ny back:", [v.hex() for v in gy])
    assert np.array_equal(gx, _through_f32(x))
    assert np.array_equal(gy, _through_f32(y))
    assert not np.array_equal(gx, x) and not np.array_equal(gy, y)


def _world1_outputs(x, y, xo, params, N, d, nb):
    g = multi_gpu.NativeDistributedGP(N, d, dtype_id=_lib.F32, nb=nb, backend="callbacks", device=0)
    try:
        g.set_data(x, y)
        out = {"log_lh": np.array(g.fit(params, 1.0))}
        out.update(alpha=g.alpha, mean=g.mean(params, xo), cov=g.cov(params, xo), var=g.var(params, xo))
        return out
    finally:
        g.close()


def test_distributed_fp32_handle_sees_the_float32_rounding_of_its_inputs():
    N, d, nb, m = 130, 2, 64, 37
    X, y, Xo = orc.synth_inputs(N, d, m)
    X, y, Xo = X.copy(), y.copy(), Xo.copy()
    X.ravel()[:4] = AWKWARD
    y[-4:] = AWKWARD
    Xo.ravel()[3:7] = AWKWARD
    for a in (X, y, Xo):                                             # the synthetic values are no float32 numbers either
        assert (a != _through_f32(a)).mean() > 0.9
    params = np.array([1.0, 0.5 * np.sqrt(d)])
    raw = _world1_outputs(X, y, Xo, params, N, d, nb)
    pre = _world1_outputs(_through_f32(X), _through_f32(y), _through_f32(Xo), params, N, d, nb)
    assert np.isfinite(raw["log_lh"]) and raw["cov"].shape == (m, m) and raw["var"].shape == (m,)
    for k in ("log_lh", "alpha", "mean", "cov", "var"):
        assert np.array_equal(raw[k], pre[k]), k


def test_world3_narrow_blocks_with_a_ragged_last_block_column():
    """nb = 64 is the one width whose trailing update takes syrk_bc's generic route; N = 209 leaves a ragged fourth block
    column whose padding columns have no rows in the panel buffer (the product has to stop at column n)."""
    from _thread_world import run_thread_world
    N, d, nb, m = 209, 2, 64, 37
    res = run_thread_world(3, N, d, nb, m, timeout=60)
    X, y, Xo = orc.synth_inputs(N, d, m)
    o = orc.OracleGP("gaussian", (1.0, 0.5 * np.sqrt(d)), X, y, 1.0)
    assert res["info"] == 0
    np.testing.assert_allclose(res["log_lh"], o.log_lh, rtol=1e-10)          # (the bounds of tests/test_gpu_round4.py's worlds)
    np.testing.assert_allclose(res["alpha"], o.inv_Kxx_y, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(res["mean"], o.mean(Xo), rtol=1e-8, atol=1e-11)
    assert res["log_lh2"] == res["log_lh"] and len(set(res["log_lh_per_rank"])) == 1


def test_fp32_ranks_that_disagree_on_chunk_rows_all_raise_and_the_next_var_succeeds():
    N, d, nb = 1000, 2, 128
    X, y, Xo = orc.synth_inputs(N, d, 300)
    params = np.array([1.0, 0.7])

    def body(rank, cb):
        g = multi_gpu.NativeDistributedGP(N, d, dtype_id=_lib.F32, nb=nb, backend="callbacks", device=0, callbacks=cb)
        try:
            g.set_data(X, y)
            g.fit(params, 1.0)
            with pytest.raises(multi_gpu.RankMismatchError, match="gpx_mg_var.*different chunk_rows"):
                g.var(params, Xo, chunk_rows=128 * rank)
            return g.var(params, Xo, chunk_rows=128)
        finally:
            g.close()

    outs = run_ranks(2, body)
    assert outs[0].shape == (300,) and np.array_equal(outs[0], outs[1])
    # (the oracle bound of tests/test_gpu_var.py::test_world2_var_fp32 for the same quantity)
    np.testing.assert_allclose(outs[1], np.diag(ref_cov("gaussian", tuple(params), X, y, 1.0, Xo)[0]), rtol=1e-2, atol=5e-3)
