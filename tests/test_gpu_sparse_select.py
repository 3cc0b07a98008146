"""GPU tests of the greedy selection of inducing points (gpx_sgp_select, csrc/gpx_select.hip; SparseGP.greedy_inducing) against
the numpy restatement of tests/_sparse_select_helpers.py, which tests/test_sparse_select_cpu.py pins.

The device's index list is not demanded to EQUAL the restatement's: after the first pick many residuals tie at exactly k(0),
and a last-bit difference may legitimately break a tie differently.  Instead the device's picks are REPLAYED in the fp64
restatement and every pick must be a valid greedy one there: its residual within tau k(0) of the largest.
tau: 1e-10 in fp64 (the project's tolerance between two evaluations of one quantity), 4 E32R[case] / k(0) in fp32 (E32R: the
fp32 restatement against the fp64 one along the same picks).  pivot, trace and R against the replay: ORACLE_TOL of
tests/test_gpu_var.py, in fp32 with the floor 4 E32R (for trace times n: it sums n residuals)."""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from test_gpu_var import ORACLE_TOL
from _sparse_helpers import S_NOISE
from _sparse_select_helpers import (CASES, CASE_IDS, E32R, FULL, ONE, SEEDS, TABLE, auto_tol, case_data, free, k0_of, make_kernel,
                                    replay)

pytestmark = pytest.mark.gpu

NP_DTYPE = {"float64": np.float64, "float32": np.float32}
DTYPE_ID = {"float64": _lib.F64, "float32": _lib.F32}
KERNEL_ID = {"gaussian": _lib.KERNEL_GAUSSIAN, "dup": _lib.KERNEL_GAUSSIAN, "periodic": _lib.KERNEL_PERIODIC, "ard": _lib.KERNEL_GAUSSIAN_ARD}
SENTINEL = -12345.0


def _tau(case, dtype):
    """The slack of a pick, as a multiple of k(0)."""
    return 1e-10 if dtype == "float64" else 4.0 * E32R[case] / k0_of(case)


def _abi(case, dtype, tol=None, first=-1, with_R=True, M=None, n=None, d=None, kernel=None):
    """gpx_sgp_select called directly: (rc, dict of the outputs cut to count, the raw arrays)."""
    x = np.ascontiguousarray(case_data(case)[0], dtype=np.float64)
    n = x.shape[0] if n is None else n
    d = (1 if x.ndim == 1 else x.shape[1]) if d is None else d
    M = case[3] if M is None else M
    rows = max(M, 1)
    tol = auto_tol(case, NP_DTYPE[dtype]) if tol is None else tol
    p = np.ascontiguousarray(case[4], dtype=np.float64)
    index = np.full(rows, int(SENTINEL), dtype=np.int64)
    pivot, trace = np.full(rows, SENTINEL), np.full(rows + 1, SENTINEL)
    R = np.full((rows, x.shape[0]), SENTINEL) if with_R else None
    count = ctypes.c_int64(int(SENTINEL))
    rc = _lib.load().gpx_sgp_select(DTYPE_ID[dtype], KERNEL_ID[case[0]] if kernel is None else kernel, _lib.dptr(x), n, d, _lib.dptr(p), M,
                                    tol, first, index.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _lib.dptr(pivot), _lib.dptr(trace),
                                    None if R is None else _lib.dptr(R), ctypes.byref(count))
    raw = dict(index=index, pivot=pivot, trace=trace, R=R, count=count.value)
    if rc != _lib.OK:
        return rc, None, raw
    c = count.value
    out = dict(index=index[:c], pivot=pivot[:c], trace=trace[:c + 1], count=c, tol=tol, R=None if R is None else R[:c])
    return rc, out, raw


_RUNS = {}


def _run(case, dtype):
    """One device run per (case, dtype) through the Python method, with the factor; shared by the tests below."""
    key = (case, dtype)
    if key not in _RUNS:
        x = case_data(case)[0]
        _lib.route_reset()
        z, info = gp.SparseGP.greedy_inducing(make_kernel(case), x, case[3], dtype=dtype, return_info=True, factor=True)
        info["routes"] = _lib.route_count(_lib.ROUTE_SELECT_STEP)
        _RUNS[key] = (z, info)
    return _RUNS[key]


def _assert_valid_picks(case, dtype, index, start=0):
    """Every pick from step `start` on is, in the fp64 replay of the list, within tau k(0) of the largest residual."""
    k0, tau = k0_of(case), _tau(case, dtype)
    rep = replay(case, index)
    worst = 0.0
    for m in range(start, len(index)):
        res = rep["res"][m]
        short = res.max() - res[index[m]]
        worst = max(worst, short / k0)
        assert short <= tau * k0, "step %d: pick %d has residual %.17g, the largest is %.17g (tau k(0) = %.3g)" % (
            m, index[m], res[index[m]], res.max(), tau * k0)
    print("%s %s: %d picks, largest shortfall %.3g k(0) (tau %.3g)" % (case[:4], dtype, len(index), worst, tau))
    return rep


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_pick_is_a_valid_greedy_pick(case, dtype):
    z, info = _run(case, dtype)
    index = info["index"]
    assert index.dtype == np.int64 and len(set(index.tolist())) == info["count"] == len(index)      # no repeated indices
    assert index.min() >= 0 and index.max() < case[1]
    _assert_valid_picks(case, dtype, index)
    # the same through the ABI: the same bits
    rc, out, _ = _abi(case, dtype)
    assert rc == _lib.OK
    for k in ("index", "pivot", "trace", "R"):
        assert np.array_equal(out[k], info[k]), k


@pytest.mark.parametrize("case", [c for c in CASES if c != ONE], ids=[i for c, i in zip(CASES, CASE_IDS) if c != ONE])
def test_index_equality_where_ties_do_not_decide(case):
    """fp64: behind the opening run of ties (residuals at exactly k(0), which both sides break by the smallest index) the
    device's picks equal the free-running restatement's for as long as its gap to the runner-up exceeds 1e-8 k(0)."""
    f, index = free(case), _run(case, "float64")[1]["index"]
    decided = f["gap"] > 1e-8 * k0_of(case)
    t0 = int(np.argmax(decided))
    end = t0 + (int(np.argmin(decided[t0:])) if not decided[t0:].all() else len(decided) - t0)
    assert decided[t0] and end - t0 >= 1                              # not vacuous
    assert sorted(index[:t0].tolist()) == sorted(f["index"][:t0].tolist())
    assert np.array_equal(index[t0:end], f["index"][t0:end])
    print("%s: %d opening ties, then %d decided picks equal" % (case[:4], t0, end - t0))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_pivot_trace_factor_and_z_against_the_replay(case, dtype):
    x = case_data(case)[0]
    z, info = _run(case, dtype)
    n, k0, count = case[1], k0_of(case), info["count"]
    rep = replay(case, info["index"])
    tol = ORACLE_TOL[dtype]
    floor = 0.0 if dtype == "float64" else 4.0 * E32R[case]
    for name, scale in (("pivot", 1.0), ("trace", float(n)), ("R", 1.0)):
        got, ref = info[name], rep[name]
        assert got.shape == ref.shape, name
        err = np.abs(got - ref)
        bound = np.maximum(tol["atol"] + tol["rtol"] * np.abs(ref), floor * scale)
        print("%s %s %s: max error %.3g (largest bound %.3g)" % (case[:4], dtype, name, err.max(), bound.max()))
        assert np.all(err <= bound), (name, float(err.max()))
    assert z.dtype == np.float64 and z.shape == (count,) + x.shape[1:]
    assert np.array_equal(z, x[info["index"]])                       # exact copies of rows of x, in the order picked
    assert info["routes"] == count
    assert info["tol"] == pytest.approx(auto_tol(case, NP_DTYPE[dtype]), rel=1e-6)      # (k(0) from the kernel class / from the oracle)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_stop_rule(case, dtype):
    z, info = _run(case, dtype)
    k0, M, count = k0_of(case), case[3], info["count"]
    assert np.all(info["pivot"] > info["tol"])
    if count < M:
        rep = replay(case, info["index"])
        assert rep["res"][-1].max() <= info["tol"] + _tau(case, dtype) * k0
    early = (case == TABLE[4]) or (dtype == "float32" and case == TABLE[3])
    assert (count < M) == early, (count, M)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_tol_zero_and_first(dtype):
    x = case_data(FULL)[0]
    K = make_kernel(FULL)
    z, info = gp.SparseGP.greedy_inducing(K, x, 40, tol=0.0, dtype=dtype, return_info=True)
    assert info["count"] == 40 and sorted(info["index"].tolist()) == list(range(40)) and info["tol"] == 0.0
    assert "R" not in info
    case = TABLE[0]
    x = case_data(case)[0]
    z, info = gp.SparseGP.greedy_inducing(make_kernel(case), x, case[3], first=17, dtype=dtype, return_info=True)
    assert info["index"][0] == 17 and info["count"] == case[3] and np.array_equal(z[0], x[17])
    _assert_valid_picks(case, dtype, info["index"], start=1)
    z2 = gp.SparseGP.greedy_inducing(make_kernel(case), x, case[3], first=17, dtype=dtype)
    assert np.array_equal(z2, z)


def test_end_to_end_bound_at_the_greedy_points():
    case = TABLE[0]
    x, y = case_data(case)
    z, info = _run(case, "float64")
    K = make_kernel(case)
    sg = gp.SparseGP(K, x, y, S_NOISE, z, jitter=0.0)
    np.testing.assert_allclose(-2.0 * sg.elbo_terms["trace"], info["trace"][-1], **ORACLE_TOL["float64"])
    sg.jitter = 1e-6
    greedy_elbo = sg.elbo
    for seed in SEEDS:
        sg.z = gp.SparseGP.subset_inducing(x, case[3], seed)
        print("seed %d: elbo %.2f (greedy: %.2f)" % (seed, sg.elbo, greedy_elbo))
        assert greedy_elbo > sg.elbo


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", [TABLE[2], TABLE[4]], ids=[CASE_IDS[2], CASE_IDS[4]])
def test_repeatability(case, dtype):
    rc1, a, _ = _abi(case, dtype)
    rc2, b, _ = _abi(case, dtype)
    rc3, c, raw = _abi(case, dtype, with_R=False)
    assert rc1 == rc2 == rc3 == _lib.OK
    for k in ("index", "pivot", "trace", "R"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("index", "pivot", "trace"):
        assert np.array_equal(a[k], c[k]), k
        assert np.all(raw[k][len(c[k]):] == SENTINEL)                # nothing behind the valid entries is written
    assert a["count"] == b["count"] == c["count"]


def test_refusals_at_the_abi():
    case = FULL
    bad = [dict(n=0), dict(M=0), dict(M=41), dict(tol=-1.0), dict(tol=np.inf), dict(tol=np.nan), dict(first=40), dict(d=0),
           dict(d=95), dict(kernel=7), dict(kernel=_lib.KERNEL_GAUSSIAN_ARD, d=_lib.ARD_MAX_D + 1)]
    for kw in bad:
        rc, out, raw = _abi(case, "float64", **kw)
        assert rc == _lib.ERR_ARG and _lib.last_error(), kw
        assert raw["count"] == int(SENTINEL), kw
        for k in ("index", "pivot", "trace", "R"):
            assert np.all(raw[k] == SENTINEL), (kw, k)               # nothing is written to the outputs
    rc, out, _ = _abi(case, "float64")
    assert rc == _lib.OK and out["count"] == 40
