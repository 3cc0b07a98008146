"""CPU tests of SparseGP's gradient of the bound: the closed form of tests/_sparse_grad_helpers.py against central differences
of the bound of tests/_sparse_helpers.py, `SparseGP.optimize` with the device replaced by that numpy restatement, and the
binding of the new symbols.

Measured ratios |closed - fd| / (1 + |closed|) (bound 1e-6; step 1e-5 theta_p, fp64), the largest over both jitters:
gaussian cases <= 2.2e-9, periodic (777, 1, 64) 1.0e-7, ard (1000, 3, 200) 3.4e-10 -- the rectangular ARD derivative is new
here and agrees as the oracle's Jacobians do."""
from ctypes import POINTER, byref, c_double, c_float, c_int, c_int64, c_size_t, c_void_p
import re

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from conftest import ROOT
from _sparse_helpers import CASES, CASE_IDS, S_NOISE, case_data, case_jitter, make_kernel, sgpr_reference
from _sparse_grad_helpers import ARD_RUNG_KEYS, median_kernel_ratio, sgpr_grad_reference


@pytest.mark.parametrize("jitter_of", [np.float64, np.float32], ids=["jitter64", "jitter32"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_closed_form_against_central_differences(case, jitter_of):
    kind = case[0]
    params, x, y, z, _, _ = case_data(case)
    jitter = case_jitter(case, jitter_of)                 # held fixed: it is not differentiated
    theta = np.array(tuple(params) + (S_NOISE,), dtype=np.float64)
    closed, scale = sgpr_grad_reference(kind, params, x, y, z, S_NOISE, jitter, np.float64)
    assert closed.shape == scale.shape == theta.shape and np.isfinite(closed).all() and (scale > 0).all()

    def bound(t):
        return float(sgpr_reference(kind, tuple(t[:-1]), x, y, z, t[-1], jitter, np.float64)["elbo"])

    worst = 0.0
    for p in range(theta.size):
        step = 1e-5 * theta[p]
        up, dn = theta.copy(), theta.copy()
        up[p] += step
        dn[p] -= step
        fd = (bound(up) - bound(dn)) / (2.0 * step)
        ratio = abs(closed[p] - fd) / (1.0 + abs(closed[p]))
        worst = max(worst, ratio)
        print("theta[%d]: closed %+.9e  fd %+.9e  |closed - fd| / (1 + |closed|) = %.2e  (scale %.2e)" % (p, closed[p], fd, ratio, scale[p]))
        assert abs(closed[p] - fd) <= 1e-6 * (1.0 + abs(closed[p])), p
    print("%s jitter %.3e: largest ratio %.2e" % (CASE_IDS[CASES.index(case)], jitter, worst))


def test_ard_rung_shapes_have_entries_that_count():
    """The ARD shapes of the GPU test's DMAX = 16, 32, 64 rungs: half the rectangle's entries are at least 1e-5 k(0).  With
    entries that underflow only coincident points contribute, their t_k are zero, and the S_k sums of the rectangular
    pass would be exactly zero whatever the kernel computes."""
    assert [k[2] for k in ARD_RUNG_KEYS] == [9, 17, 33]
    for key in ARD_RUNG_KEYS:
        med = median_kernel_ratio(key)
        print("%s: median k / k(0) = %.2e" % (key, med))
        assert med >= 1e-5, key


# ---- optimize() with the numpy restatement in place of the device ----------------------------------------------------------
class _NumpySparse(gp.SparseGP):
    """SparseGP whose one hook into the device is the numpy restatement; `fail_on`: the call that reports a failed fit."""
    KIND = "gaussian"
    calls = 0
    fail_on = None

    def elbo_and_grad(self):
        self.calls += 1
        self.seen.append(self.params)
        if self.calls == self.fail_on:
            return -np.inf, np.full(self.params.size, np.nan)
        p = self.params
        val = float(sgpr_reference(self.KIND, tuple(p[:-1]), self.x, self.y, self.z, p[-1], self.jitter)["elbo"])
        grad = sgpr_grad_reference(self.KIND, tuple(p[:-1]), self.x, self.y, self.z, p[-1], self.jitter)[0]
        self.values.append(val)
        return val, grad


def _numpy_sparse(monkeypatch, fail_on=None):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    case = CASES[5]
    assert case == ("gaussian", 300, 3, 300)
    params, x, y, z, _, _ = case_data(case)
    sg = _NumpySparse(make_kernel(case[0], case[2]), x, y, S_NOISE, z, jitter=case_jitter(case, np.float64))
    sg.seen, sg.values, sg.fail_on = [], [], fail_on
    start = sg.params * np.array([1.5, 0.7, 1.3])
    sg.params = start
    p = sg.params
    at_start = float(sgpr_reference("gaussian", tuple(p[:-1]), x, y, z, p[-1], sg.jitter)["elbo"])
    return sg, at_start


def test_optimize_improves_the_bound_and_leaves_the_best_parameters(monkeypatch):
    sg, at_start = _numpy_sparse(monkeypatch)
    res = sg.optimize(maxiter=10)
    assert set(res) == {"params", "elbo", "nit", "nfev", "success", "message"}
    print("start %.6f -> %.6f in %d iterations, %d evaluations: %s" % (at_start, res["elbo"], res["nit"], res["nfev"], res["message"]))
    assert res["elbo"] >= at_start
    assert res["elbo"] == max(sg.values)
    assert np.array_equal(sg.params, res["params"])
    assert sg.calls == res["nfev"]                                   # one elbo_and_grad per evaluation
    assert any(np.array_equal(res["params"], p) for p in sg.seen)
    assert res["nit"] <= 10 and isinstance(res["success"], bool) and isinstance(res["message"], str)


def test_optimize_survives_a_failed_fit(monkeypatch):
    sg, at_start = _numpy_sparse(monkeypatch, fail_on=3)
    res = sg.optimize(maxiter=6)
    assert sg.calls >= 3                                             # the failure happened and the run went on
    print("start %.6f -> %.6f, %d evaluations (the third failed)" % (at_start, res["elbo"], sg.calls))
    assert np.isfinite(res["elbo"]) and res["elbo"] >= at_start
    assert np.array_equal(sg.params, res["params"])


def test_optimize_bounds(monkeypatch):
    sg, _ = _numpy_sparse(monkeypatch)
    with pytest.raises(ValueError):
        sg.optimize(bounds=[(0.1, 10.0)])
    start = sg.params
    res = sg.optimize(maxiter=3, bounds=[(0.5 * v, 1.02 * v) for v in start])
    assert np.all(res["params"] >= 0.5 * start * (1 - 1e-12)) and np.all(res["params"] <= 1.02 * start * (1 + 1e-12))


def test_gradient_symbols_are_bound():
    want = {
        "gpx_sgp_grad": (c_int, [c_void_p, c_int64, POINTER(c_double)]),
        "gpx_sgp_last_grad_timing": (c_int, [c_void_p, POINTER(c_float)]),
    }
    with open(ROOT + "/include/gpx.h") as f:
        hdr = f.read()
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name][0] is res
        assert list(_lib._SIGNATURES[name][1]) == args, name
    assert re.search(r"int gpx_sgp_grad\(gpx_sgp_t \*h, int64_t chunk_cols, double \*grad\);", hdr)
    assert re.search(r"int gpx_sgp_last_grad_timing\(gpx_sgp_t \*h, float \*ms5\);", hdr)
    assert _lib.PROF_SPARSE_GRAD == 20 and re.search(r"#define GPX_PROF_SPARSE_GRAD\s+20\b", hdr)
    lib = _lib.load()                                                # (resolves both in the built library)
    assert lib.gpx_sgp_grad.argtypes == want["gpx_sgp_grad"][1]
    for name in ("delbo_dtheta", "elbo_and_grad", "grad_timing", "optimize"):
        assert hasattr(gp.SparseGP, name)
    assert "optimize" not in gp.__all__ and not hasattr(gp, "delbo_dtheta")


# ---- the plan of a gradient pass: host arithmetic (no GPU) ----
def _plans(n, M, chunk_cols=0, free=1 << 36, dtype=_lib.F64):
    """(rc, (cols, chunks)) of the gradient's plan and of the fit's, for the same arguments."""
    lib, out = _lib.load(), []
    for entry, extra in ((lib.gpx_debug_sgp_plan, (None, None)), (lib.gpx_debug_sgp_grad_plan, ())):
        cols, chunks = c_int64(0), c_int64(0)
        rc = entry(dtype, n, M, chunk_cols, 0, free, byref(cols), byref(chunks), *extra)
        out.append((rc, (cols.value, chunks.value)))
    return out[::-1]                                                  # (the gradient's ran last: last_error() is its)


def test_plan_of_a_gradient_pass():
    """Two cols x ldm blocks where the fit holds one M x cols: fp64, n = 2^20, M = ldm = 4096."""
    n, M = 1 << 20, 4096
    assert _plans(n, M, free=1 << 36) == [(_lib.OK, (16384, 64))] * 2                 # 2^30 bytes within the quarter: the fit's plan
    # the fit takes 8192 columns; two blocks of 8192 x 4096 doubles are 2^29 bytes, the quarter 2^28: halved once, 2^28 fits
    assert _plans(n, M, free=1 << 30) == [(_lib.OK, (4096, 256)), (_lib.OK, (8192, 128))]
    grad, fit = _plans(n, M, chunk_cols=8192, free=1 << 30)                            # explicit chunks are never halved
    assert grad[0] == _lib.ERR_NOMEM and "two blocks of 8192 columns" in _lib.last_error()
    assert fit == (_lib.OK, (8192, 128))
    assert _plans(1000, 128, chunk_cols=128) == [(_lib.OK, (128, 8))] * 2
    for bad in (100, 129, -128):
        for rc, _ in _plans(1000, 128, chunk_cols=bad):
            assert rc == _lib.ERR_ARG and "chunk_cols" in _lib.last_error()


def test_gradient_plan_symbol_is_bound():
    want = (c_int, [c_int, c_int64, c_int64, c_int64, c_int, c_size_t, POINTER(c_int64), POINTER(c_int64)])
    assert "gpx_debug_sgp_grad_plan" in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGNATURES["gpx_debug_sgp_grad_plan"][0] is want[0]
    assert list(_lib._SIGNATURES["gpx_debug_sgp_grad_plan"][1]) == want[1]
    with open(ROOT + "/include/gpx.h") as f:
        hdr = f.read()
    assert re.search(r"int gpx_debug_sgp_grad_plan\(int dtype, int64_t n, int64_t m_inducing, int64_t chunk_cols, int split, "
                     r"size_t free_bytes,\s+int64_t \*cols, int64_t \*chunks\);", hdr)
    assert _lib.load().gpx_debug_sgp_grad_plan.argtypes == want[1]
