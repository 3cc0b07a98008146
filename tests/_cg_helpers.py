"""Shared pieces of the tests of IterativeGP / gpx_cg_*: a numpy restatement of the algorithm the device runs (include/gpx.h,
"exact GP past the n x n factor") and the problem table.

    partial_cholesky   the pivoted partial Cholesky of K: p = argmax of the residual diagonal among the unpicked (ties: the
                       smallest index), stop when it is <= tol, R[m] = (K[p] - sum_j R[j, p] R[j]) / sqrt(dres[p])
    woodbury           P^-1 V = (V - (V R^T) C^-1 R) / s^2,  C = s^2 I + R R^T,  for P = R^T R + s^2 I; V holds vectors as rows
    pcg                batched preconditioned CG on (K + s^2 I) with the device's freezing rule: a column is frozen at the
                       iteration where rr <= tol^2 bb (its x no longer changes), from the start when b = 0 (x = 0, 0
                       iterations, relres 0), and with a negative count when delta <= 0 or is not finite

Kernel values come from oracle.gp_oracle.kernel_matrix, as in tests/_sparse_helpers.py.  tests/test_cg_cpu.py pins the
restatement and the conditions on the table that tests/test_gpu_cg.py relies on.
"""
import numpy as np

import gaussian_processes_amd as gp
from oracle import gp_oracle as orc
from _sparse_helpers import oracle_view, prior_var

EPS = np.finfo(np.float64).eps
TOL = float(np.sqrt(EPS))
MAXITER = 200
M_TEST = 70                                   # 32 + 32 + 6: the variance ends on a ragged last group

# name: kind, n, d, kernel parameters, s, rank.  n is never a multiple of 128 or 256.
PROBLEMS = {
    "A": ("gaussian", 700, 3, (1.3, 0.7), 0.2, 64),
    "B": ("periodic", 257, 1, (1.0, 0.8, 0.3), 0.3, 32),
    "C": ("ard", 515, 5, (1.2, 0.3, 0.45, 0.7, 1.0, 1.6), 0.25, 48),
    "D": ("gaussian", 12289, 2, (1.0, 0.15), 0.3, 128),
}
SMALL = ("A", "B", "C")


def make_kernel(name):
    kind, _, _, p, _, _ = PROBLEMS[name]
    if kind == "gaussian":
        return gp.GaussianKernel(*p)
    if kind == "periodic":
        return gp.PeriodicKernel(*p)
    return gp.GaussianARDKernel(p[0], list(p[1:]))


_DATA, _KXX, _REF = {}, {}, {}


def data(name):
    """(x, y, xo): x uniform in the unit cube ((n,) for d = 1), y a smooth function plus noise, xo M_TEST test points; read-only."""
    if name not in _DATA:
        _, n, d, _, _, _ = PROBLEMS[name]
        rng = np.random.RandomState(1000 + ord(name))
        x = rng.uniform(0.0, 1.0, (n, d))
        y = np.sin(2.0 * np.pi * x.sum(axis=1) / np.sqrt(d)) + 0.5 * np.cos(3.0 * x[:, 0]) + 0.1 * rng.randn(n)
        xo = rng.uniform(0.0, 1.0, (M_TEST, d))
        if d == 1:
            x, xo = x.ravel(), xo.ravel()
        for a in (x, y, xo):
            a.flags.writeable = False
        _DATA[name] = (x, y, xo)
    return _DATA[name]


def kernel_between(name, a, b):
    """K(a, b) from the oracle's kernel functions."""
    kind, _, _, p, _, _ = PROBLEMS[name]
    okind, op, av, bv = oracle_view(kind, p, a, b)
    return orc.kernel_matrix(okind, "K", av, bv, op)


def kxx(name):
    """K(x, x) of a small problem, read-only."""
    if name not in _KXX:
        assert name in SMALL
        x = data(name)[0]
        K = kernel_between(name, x, x)
        K.flags.writeable = False
        _KXX[name] = K
    return _KXX[name]


def k0_of(name):
    return prior_var(PROBLEMS[name][0], PROBLEMS[name][3])


def select_tol(name):
    """The selection's automatic tolerance: sqrt(eps) k(0)."""
    return TOL * k0_of(name)


def kappa(name):
    """lambda_max / lambda_min of K + s^2 I: from the matrix for the small problems, the bound (n k0 + s^2) / s^2 for D."""
    _, n, _, _, s, _ = PROBLEMS[name]
    if name not in SMALL:
        return (n * k0_of(name) + s * s) / (s * s)
    w = np.linalg.eigvalsh(kxx(name) + s * s * np.eye(n))
    return float(w[-1] / w[0])


def partial_cholesky(K, rank, tol):
    """(R (count, n), index): the pivoted partial Cholesky of the matrix K in the device's steps."""
    n = K.shape[0]
    dres = np.diag(K).copy()
    picked = np.zeros(n, dtype=bool)
    R = np.zeros((rank, n))
    index = []
    for m in range(rank):
        p = int(np.argmax(np.where(picked, -np.inf, dres)))      # (the first maximum: the smallest index)
        if not dres[p] > tol:
            break
        acc = np.zeros(n)
        for j in range(m):
            acc += R[j, p] * R[j]
        R[m] = (K[p] - acc) / np.sqrt(dres[p])
        dres = dres - R[m] * R[m]
        picked[p] = True
        index.append(p)
    return R[:len(index)], np.array(index, dtype=np.int64)


def woodbury(R, s, V):
    """(R^T R + s^2 I)^-1 applied to the rows of V; R with no rows: V itself (P = I)."""
    V = np.atleast_2d(V)
    if R.shape[0] == 0:
        return V.copy()
    C = s * s * np.eye(R.shape[0]) + R @ R.T
    return np.stack([(v - np.linalg.solve(C, R @ v) @ R) / (s * s) for v in V])      # (row by row, as pcg's products)


def kappa_precond(R, s):
    """Condition number of P = R^T R + s^2 I (n > rows of R): (s^2 + lambda_max(R R^T)) / s^2."""
    return float((s * s + np.linalg.eigvalsh(R @ R.T)[-1]) / (s * s))


def pcg(A, B, R, s, tol=TOL, maxiter=MAXITER):
    """Batched PCG on the matrix A (= K + s^2 I) for the rows of B with P = R^T R + s^2 I.  Returns a dict: X (S, n),
    iterations (S,), relres (S,) of the recurrence, frozen (S,) and its (the iterations the batch ran)."""
    B = np.atleast_2d(np.asarray(B, dtype=np.float64))
    S, n = B.shape
    X = np.zeros((S, n))
    r = B.copy()
    bb = (B * B).sum(axis=1)
    rr = bb.copy()
    frozen = bb == 0.0
    iters = np.zeros(S, dtype=np.int64)
    z = woodbury(R, s, r)
    rho = (r * z).sum(axis=1)
    p = z.copy()
    it = 0
    while it < maxiter and not frozen.all():
        it += 1
        q = np.stack([A @ pi for pi in p])                        # (a product per column: a column's bits do not depend on its companions)
        delta = (p * q).sum(axis=1)
        bad = ~frozen & ~((delta > 0.0) & np.isfinite(delta))
        frozen = frozen | bad
        iters[bad] = -it
        live = ~frozen
        alpha = np.zeros(S)
        alpha[live] = rho[live] / delta[live]
        X[live] += alpha[live, None] * p[live]
        r[live] -= alpha[live, None] * q[live]
        rr[live] = (r[live] * r[live]).sum(axis=1)
        done = live & (rr <= tol * tol * bb)
        frozen = frozen | done
        iters[done] = it
        if it == maxiter or frozen.all():
            break
        z = woodbury(R, s, r)
        rho_new = (r * z).sum(axis=1)
        live = ~frozen
        beta = np.zeros(S)
        nz = live & (rho != 0.0)
        beta[nz] = rho_new[nz] / rho[nz]
        rho[live] = rho_new[live]
        p[live] = z[live] + beta[live, None] * p[live]
    iters[~frozen] = it
    relres = np.where(bb > 0.0, np.sqrt(rr / np.where(bb > 0.0, bb, 1.0)), 0.0)
    return dict(X=X, iterations=iters, relres=relres, frozen=frozen, its=it)


def easy_rhs():
    """A right-hand side on A that converges well before y does without a preconditioner, with a SHARP crossing:
    (K + s^2 I) sin(3 x_0), whose solution is smooth.  (A column of K also converges early, but its residual creeps across
    tol: perturbing b by 1e-15 moves the restatement's own count between 43 and 47; this one stays at 36.)"""
    x = data("A")[0]
    return reference("A", 0)["A"] @ np.sin(3.0 * x[:, 0])


def true_relres(A, x, b):
    """|b - A x| / |b| formed in numpy."""
    return float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))


def reference(name, rank=None):
    """The restatement on a small problem's own y, one evaluation per (problem, rank): A = K + s^2 I, R, the pcg record, kappa."""
    _, n, _, _, s, prank = PROBLEMS[name]
    rank = prank if rank is None else rank
    key = (name, rank)
    if key not in _REF:
        x, y, _ = data(name)
        A = kxx(name) + s * s * np.eye(n)
        R, index = partial_cholesky(kxx(name), rank, select_tol(name)) if rank > 0 else (np.zeros((0, n)), np.zeros(0, dtype=np.int64))
        rec = pcg(A, y, R, s)
        rec.update(A=A, R=R, index=index, true_relres=true_relres(A, rec["X"][0], y))
        _REF[key] = rec
    return _REF[key]
