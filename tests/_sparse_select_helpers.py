"""Shared pieces of the tests of SparseGP.greedy_inducing / gpx_sgp_select: a numpy restatement of greedy conditional-variance
selection (a pivoted partial Cholesky of K(x, x)) in the five steps the device runs (include/gpx.h, gpx_sgp_select), the test
cases, and the fp32 error scale of every case.

    dres[i] = k(x_i, x_i);  step m:  p = argmax over the unpicked (ties: the smallest index; step 0: `first` when given)
    stop when dres[p] <= tol;  R[m] = (k(x_p, .) - sum_{j < m} R[j, p] R[j]) / sqrt(dres[p]), j ascending, rounded to `dtype`
    dres -= R[m]^2;  p is picked, its residual counts as 0;  trace[m + 1] = sum over the unpicked of dres

Two modes: free (it picks for itself) and replay (it follows a given index list; it stops only when a tolerance is given
explicitly).  Either way it returns the residual vector before every pick and after the last one.  tests/test_sparse_select_cpu.py pins the restatement;
tests/test_gpu_sparse_select.py leans on it.  Kernel values come from oracle.gp_oracle.kernel_matrix, evaluated in float64
and cast, as in tests/_sparse_helpers.py; all sums are float64 for both dtypes.
"""
import numpy as np

import gaussian_processes_amd as gp
from oracle import gp_oracle as orc
from _sparse_helpers import oracle_view, prior_var, sgpr_reference, S_NOISE, JITTER64

# kind, N, d, M, kernel parameters.  "dup": 300 rows with the first 100 appended again, permuted by RandomState(5)
TABLE = [("gaussian", 1500, 2, 96, (1.0, 2.0)), ("ard", 1200, 3, 160, (1.0, 2.0, 3.0, 4.5)), ("gaussian", 4099, 2, 130, (1.0, 1.5)),
         ("gaussian", 777, 1, 48, (1.3, 0.6)), ("periodic", 777, 1, 24, (0.8, 1.0, 5.0))]
FULL = ("gaussian", 40, 2, 40, (1.0, 2.0))                # M = N
ONE = ("gaussian", 777, 1, 1, (1.3, 0.6))                 # M = 1
DUP = ("dup", 400, 2, 60, (1.0, 2.0))
CASES = TABLE + [FULL, ONE, DUP]
CASE_IDS = ["%s-%d-%d-%d" % c[:4] for c in CASES]
WELL = TABLE[:3]                                          # last pivot > 1e-2 k(0); greedy beats every random subset by >= 2.7
FP64_PICKS = {TABLE[0]: 96, TABLE[1]: 160, TABLE[2]: 130, TABLE[3]: 48, TABLE[4]: 16, FULL: 40, ONE: 1, DUP: 60}
SEEDS = (0, 1, 2, 3, 4)


def kind_of(case):
    return "gaussian" if case[0] == "dup" else case[0]


def make_kernel(case):
    kind, p = kind_of(case), case[4]
    if kind == "gaussian":
        return gp.GaussianKernel(*p)
    if kind == "periodic":
        return gp.PeriodicKernel(*p)
    return gp.GaussianARDKernel(p[0], list(p[1:]))


_DATA = {}


def case_data(case):
    """(x, y): 1-D inputs are (n,) arrays; read-only."""
    if case not in _DATA:
        kind, N, d, _, _ = case
        if kind == "dup":
            X, y, _ = orc.synth_inputs(300, d, 1)
            perm = np.random.RandomState(5).permutation(400)
            X, y = np.concatenate([X, X[:100]])[perm], np.concatenate([y, y[:100]])[perm]
        else:
            X, y, _ = orc.synth_inputs(N, d, 1)
        if d == 1:
            X = X.ravel()
        X, y = np.ascontiguousarray(X), np.ascontiguousarray(y)
        X.flags.writeable = False
        y.flags.writeable = False
        _DATA[case] = (X, y)
    return _DATA[case]


def k0_of(case):
    return prior_var(kind_of(case), case[4])


def auto_tol(case, dtype):
    """greedy_inducing's tol=None: sqrt(eps_dtype) * k(0)."""
    return float(np.sqrt(np.finfo(dtype).eps) * k0_of(case))


def greedy(case, dtype=np.float64, tol=None, first=None, replay=None, M=None):
    """The restatement.  Free mode (replay is None): picks up to M (default: the case's) points and stops by `tol` (default: the
    automatic one of `dtype`).  Replay mode: follows the index list `replay`; no stop rule unless `tol` is given.
    Returns index, pivot, trace (count + 1), R (count, n; float64 values rounded to `dtype`), count, tol, res ((count + 1, n):
    the residuals before every pick and after the last, picked points at 0) and gap (per pick: its residual minus the
    runner-up's, the largest among the other unpicked points; inf when there is none)."""
    x, _ = case_data(case)
    okind, op, xv = oracle_view(kind_of(case), case[4], x)
    xv = xv.reshape(x.shape[0], -1)
    n = xv.shape[0]
    T = np.dtype(dtype).type
    M = (case[3] if M is None else int(M)) if replay is None else len(replay)
    stops = replay is None or tol is not None
    tol = auto_tol(case, dtype) if tol is None else float(tol)
    dres = np.full(n, np.float64(T(k0_of(case))))
    picked = np.zeros(n, dtype=bool)
    R = np.zeros((M, n))
    index, pivot, gap, trace, res = [], [], [], [dres.sum()], []
    for m in range(M):
        cur = np.where(picked, 0.0, dres)
        res.append(cur)
        cand = np.where(picked, -np.inf, dres)
        if replay is not None:
            p = int(replay[m])
        elif m == 0 and first is not None:
            p = int(first)
        else:
            p = int(np.argmax(cand))                      # (the first maximum: the smallest index)
        if stops and not dres[p] > tol:
            break
        others = cand.copy()
        others[p] = -np.inf
        gap.append(dres[p] - others.max() if n > m + 1 else np.inf)
        k = orc.kernel_matrix(okind, "K", xv[p:p + 1], xv, op)[0].astype(T).astype(np.float64)
        acc = np.zeros(n)
        for j in range(m):
            acc += R[j, p] * R[j]
        R[m] = ((k - acc) / np.sqrt(dres[p])).astype(T).astype(np.float64)
        index.append(p)
        pivot.append(dres[p])
        dres = dres - R[m] * R[m]
        picked[p] = True
        trace.append(dres[~picked].sum())
    count = len(index)
    res = res[:count] + [np.where(picked, 0.0, dres)]
    return dict(index=np.array(index, dtype=np.int64), pivot=np.array(pivot), trace=np.array(trace), R=R[:count], count=count, tol=tol,
                res=np.array(res), gap=np.array(gap))


_FREE, _REPLAY = {}, {}


def free(case, dtype=np.float64):
    """The free run of a case at its automatic tolerance, one evaluation per (case, dtype)."""
    key = (case, np.dtype(dtype).name)
    if key not in _FREE:
        _FREE[key] = greedy(case, dtype)
    return _FREE[key]


def replay(case, index, dtype=np.float64):
    """The replay of an index list, one evaluation per (case, list, dtype)."""
    key = (case, tuple(int(i) for i in index), np.dtype(dtype).name)
    if key not in _REPLAY:
        _REPLAY[key] = greedy(case, dtype, replay=key[1])
    return _REPLAY[key]


class _E32R(dict):
    """E32R[case]: the largest |fp32 replay - fp64 replay| of a residual along the fp64 picks; filled on first use.  The fp32
    replay ends where an fp32 run would: at the first of those picks whose fp32 residual is not above the fp32 tolerance
    (beyond it an fp32 residual may be negative and has no square root: the periodic case, whose fp64 run goes on to pivots of
    1.8e-8 k(0)); the residuals up to and including that step are compared."""

    def __missing__(self, case):
        f64 = free(case)
        r32 = greedy(case, np.float32, tol=auto_tol(case, np.float32), replay=f64["index"])
        steps = r32["count"] + 1
        self[case] = float(np.abs(r32["res"][:steps] - f64["res"][:steps]).max())
        return self[case]


E32R = _E32R()


def elbo_at(case, z, jitter=JITTER64):
    """The restated bound (tests/_sparse_helpers.sgpr_reference) of the case's data at inducing inputs z, s = 1."""
    x, y = case_data(case)
    return sgpr_reference(kind_of(case), case[4], x, y, z, S_NOISE, jitter)
