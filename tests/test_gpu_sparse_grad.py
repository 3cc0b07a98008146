"""GPU tests of SparseGP's gradient of the bound (gpx_sgp_grad, csrc/gpx_sparse.hip; the rectangular tile reduction of
csrc/gpx_kmat.hip) against the closed form of tests/_sparse_grad_helpers.py, which tests/test_sparse_grad_cpu.py pins against
central differences of the bound.

Tolerances.  fp64 (jitter 1e-6): ORACLE_TOL["float64"] (rtol 1e-7, atol 1e-10), or C_COND cond(Kuu) eps scale_p where that is
larger -- the convention of tests/test_gpu_ard._nclose with the project's C_COND = 16 and the scale_p of the helper (the size of
the terms that enter component p).  fp32 (automatic jitter): ORACLE_TOL["float32"] with the floor 4 E32G, E32G the distance
between the fp32 and the fp64 run of the restatement at the fp32 jitter: the rule of tests/test_gpu_sparse.py.  Every test
prints error, bound and floor per component.
Shapes: (N, M) at the edges of the 64-tile and of a 128-column chunk (chunk_cols = 128: 2 and 3 chunks with ragged last chunks
of 1 and 44 columns), all three families, ARD at d = 9, 17, 33 (the DMAX = 16, 32, 64 rungs of the rectangular pass; widths
at which the rectangle's entries are not all zero: ARD_RUNG_KEYS) at 129 x 65; the six cases of tests/_sparse_helpers.py
at automatic chunking, the first of them under its depth-slice plans as well."""
import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from test_gpu_var import C_COND, ORACLE_TOL
from _sparse_helpers import CASES, CASE_IDS, PLANS_N1000, S_NOISE, case_data, case_jitter
from _sparse_grad_helpers import ARD_RUNG_KEYS, E32G, EDGE_PAIRS, grad_reference, make_kernel, problem

pytestmark = pytest.mark.gpu

_EPS = float(np.finfo(np.float64).eps)
EDGE_KEYS = [(kind, N, d, M) for N, M in EDGE_PAIRS for kind, d in (("gaussian", 3), ("periodic", 1), ("ard", 3))] + ARD_RUNG_KEYS
EDGE_IDS = ["%s-%d-%d-%d" % k for k in EDGE_KEYS]
START = np.array([1.5, 0.7, 1.3])


def _chunks(N, chunk_cols):
    return 1 if chunk_cols == 0 else -(-N // chunk_cols)          # automatic: every shape here fits one chunk


def _sparse(key, dtype="float64", chunk_cols=0):
    params, x, y, z = problem(key)
    jitter = 1e-6 if dtype == "float64" else None
    return gp.SparseGP(make_kernel(key[0], params), x, y, S_NOISE, z, jitter=jitter, dtype=dtype, chunk_cols=chunk_cols)


def _assert_gradient(key, dtype, sg, got):
    ref, scale, cond = grad_reference(key, sg.jitter)
    assert got.shape == ref.shape and got.dtype == np.float64
    tol = ORACLE_TOL[dtype]
    err = np.abs(got - ref)
    bound = tol["atol"] + tol["rtol"] * np.abs(ref)
    if dtype == "float64":
        floor = C_COND * cond * _EPS * scale
    else:
        floor = 4.0 * E32G[key]
    bad = []
    for p in range(ref.size):
        ok = err[p] <= max(bound[p], floor[p])
        print("theta[%d] %+.6e  err %.3e  bound %.3e  floor %.3e  (scale %.3e, cond(Kuu) %.2e)%s"
              % (p, ref[p], err[p], bound[p], floor[p], scale[p], cond, "" if ok else "  <-- FAILS"))
        if not ok:
            bad.append(p)
    assert not bad, "components beyond tolerance: %s" % bad


@pytest.mark.parametrize("chunk_cols", [0, 128])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("key", EDGE_KEYS, ids=EDGE_IDS)
def test_parity_at_the_tile_and_chunk_edges(key, dtype, chunk_cols):
    _lib.route_reset()
    sg = _sparse(key, dtype, chunk_cols)
    got = sg.delbo_dtheta
    assert _lib.route_count(_lib.ROUTE_SPARSE_CHUNK) == 2 * _chunks(key[1], chunk_cols)     # the fit's chunks, then the gradient's
    _assert_gradient(key, dtype, sg, got)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_parity_of_the_cases(case, dtype):
    _lib.route_reset()
    sg = _sparse(case, dtype)
    if dtype == "float32":
        assert np.isclose(sg.jitter, case_jitter(case, np.float32), rtol=1e-6, atol=0.0)
    got = sg.delbo_dtheta
    assert _lib.route_count(_lib.ROUTE_SPARSE_CHUNK) == 2
    _assert_gradient(case, dtype, sg, got)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("plan", sorted(PLANS_N1000), ids=["cols%d-split%d" % p for p in sorted(PLANS_N1000)])
def test_parity_under_the_depth_slice_plans(plan, dtype):
    case = CASES[0]
    chunk_cols, split = plan
    sg = _sparse(case, dtype, chunk_cols)
    _lib.check(_lib.load().gpx_sgp_set_split(sg._state().handle, split))
    _lib.route_reset()
    got = sg.delbo_dtheta
    assert _lib.route_count(_lib.ROUTE_SPARSE_CHUNK) == 2 * PLANS_N1000[plan][0]
    _assert_gradient(case, dtype, sg, got)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case,chunk_cols", [(CASES[0], 128), (CASES[2], 0), (CASES[3], 128)], ids=["gaussian-128", "ard-auto", "periodic-128"])
def test_bits_repeat_and_the_fit_is_left_alone(case, chunk_cols, dtype):
    xo = case_data(case)[4]
    sg = _sparse(case, dtype, chunk_cols)
    before = dict(elbo=sg.elbo, mean=sg.mean(xo), var=sg.var(xo), Luu=sg.Luu.copy(), LB=sg.LB.copy(), c=sg.c.copy())
    _lib.route_reset()
    grad = sg.delbo_dtheta
    assert _lib.route_count(_lib.ROUTE_SPARSE_CHUNK) == _chunks(case[1], chunk_cols)        # the gradient pass alone: no refit
    val, g2 = sg.elbo_and_grad()
    assert val == sg.elbo and np.array_equal(g2, grad) and np.array_equal(sg.delbo_dtheta, grad)
    assert _lib.route_count(_lib.ROUTE_SPARSE_CHUNK) == _chunks(case[1], chunk_cols)        # memoised
    # the pass did not disturb what the fit left on the device: read everything again, past the memo
    sg._memoized = {}
    assert sg.elbo == before["elbo"]
    assert np.array_equal(sg.mean(xo), before["mean"]) and np.array_equal(sg.var(xo), before["var"])
    for name in ("Luu", "LB", "c"):
        assert np.array_equal(getattr(sg, name), before[name]), name
    # a second gradient of the same fit, and one of a second object on the same data: the same bytes
    assert np.array_equal(sg.delbo_dtheta, grad)
    assert _lib.route_count(_lib.ROUTE_SPARSE_CHUNK) == 2 * _chunks(case[1], chunk_cols)
    assert np.array_equal(_sparse(case, dtype, chunk_cols).delbo_dtheta, grad)
    # a setter invalidates it
    sg.s = 1.25
    assert not np.array_equal(sg.delbo_dtheta, grad)
    t = sg.grad_timing()
    assert set(t) == {"mm", "build", "product", "reduce", "total"} and all(v >= 0 for v in t.values())
    assert t["total"] >= max(t["mm"], t["build"], t["product"], t["reduce"])


def test_optimize_on_the_device():
    case = CASES[0]
    sg = _sparse(case)
    sg.params = sg.params * START
    at_start = sg.elbo
    seen = []
    inner = sg.elbo_and_grad

    def spy():
        out = inner()
        seen.append(out[0])
        return out
    sg.elbo_and_grad = spy
    res = sg.optimize(maxiter=15)
    print("start %.6f -> %.6f in %d iterations, %d evaluations: %s" % (at_start, res["elbo"], res["nit"], res["nfev"], res["message"]))
    assert len(seen) == res["nfev"]
    assert res["elbo"] >= at_start
    assert res["elbo"] >= max(v for v in seen if np.isfinite(v))
    assert res["elbo"] == sg.elbo and np.array_equal(res["params"], sg.params)


def test_failed_factorisation():
    case = CASES[4]
    _, x, y, z, _, _ = case_data(case)
    zz = np.array(z)
    zz[12:] = zz[:12]                                                # every inducing point twice, no jitter: Kuu has rank 12
    sg = gp.SparseGP(make_kernel(case[0], problem(case)[0]), x, y, S_NOISE, zz, jitter=0.0)
    st = sg._fit()
    assert st.stage == 1
    with pytest.raises(np.linalg.LinAlgError, match=r"stage 1 .*%d-th leading minor" % st.pivot):
        sg.delbo_dtheta
    val, grad = sg.elbo_and_grad()
    assert val == -np.inf and grad.shape == (3,) and np.isnan(grad).all()
    grad_buf = np.zeros(3)
    assert _lib.load().gpx_sgp_grad(st.handle, 0, _lib.dptr(grad_buf)) == _lib.ERR_ARG
    sg.z = z                                                         # a good fit on the same object
    sg.jitter = 1e-6
    assert np.array_equal(sg.delbo_dtheta, _sparse(case).delbo_dtheta)
