"""Shared pieces of the tests of IterativeGP's marginal-likelihood estimate (gpx_cg_lh, gpx_cg_probes, gpx_d_lowrank_reduce): a
numpy restatement of what the device runs, on the problems of tests/_cg_helpers.py, and the dense references it is pinned to.

    pcg_record       tests/_cg_helpers.pcg with the device's record: the step lengths alpha_j and ratios beta_j of every
                     column (0 once the column is frozen), rho0 = z . P^-1 z and Zt = P^-1 z
    quadrature       e1^T log(T) e1 of the Lanczos tridiagonal of one column's coefficients:
                     T[j, j] = 1 / alpha_j + beta_{j-1} / alpha_{j-1},  T[j, j+1] = sqrt(beta_j) / alpha_j
    estimate         the per-probe terms rho0_t e1^T log(T_t) e1 and log det P + their mean
    dense references probe_terms: u^T log(P^-1/2 (K + s^2 I) P^-1/2) u with u = P^-1/2 z, per probe (an eigendecomposition);
                     logdet: slogdet(K + s^2 I); lowrank_sums: sum c_ji dk_p and its magnitude sum |c_ji dk_p|, in the slots of
                     the dense gradient's reduction; dense_grad: 1/2 tr((alpha alpha^T - (K + s^2 I)^-1) dK_p) from the oracle's
                     derivative matrices (the ARD family: from its closed form on the scaled points)

Q_TOL[name] is 100 x the restatement's own worst per-probe error against probe_terms on that problem PER UNIT OF rho0 = z . P^-1 z,
measured on the CPU (tests/test_cg_lh_cpu.py prints the figures and asserts that the restatement stays a factor 100 inside).
The rows of P^1/2 have rho0 = 1 and terms of size 1 to 3; a probe scaled by c has its term, and its error, scaled by c^2, so a
bound on a probe is Q_TOL rho0.  The exact-trace probes are sqrt(n) P^1/2 (sqrt(n) I at rank 0): their second moment
Z^T Z / T is P itself, so the estimate's mean over the T = n probes is the trace, and each term carries rho0 = n.
"""
import numpy as np

from oracle import gp_oracle as orc
from _ard_helpers import iso_params
from _cg_helpers import MAXITER, PROBLEMS, TOL, data, reference, woodbury
from _sparse_helpers import oracle_view

T_GIVEN = 33                                  # 32 + 1: the given probes end on a ragged group

# 100 x the worst |restatement - dense| / rho0 over the rows of P^1/2 (at rank 0 and at the table's rank) and the 33 given
# Gaussian probes.  That error is rounding noise and moves with the summation order of numpy's products, that is with the BLAS
# thread count: over 1, 2, 4, 8 and 16 threads it was 5.6e-12 .. 6.4e-12 on A (rank 0; 1.6e-12 .. 3.2e-12 at rank 64),
# 5.3e-13 .. 7.0e-13 on B and 2.0e-13 .. 6.0e-13 on C (tests/test_cg_lh_cpu.py prints the figures).  The measured figure is the
# worst of those rounded up to the next power of ten: 1e-11, 1e-12, 1e-12.
Q_TOL = {"A": 1e-9, "B": 1e-10, "C": 1e-10}

# IterativeGP.optimize against mlii.optimize on the 200 x 2 problem of tests/test_gpu_cg_lh.py: the permitted shortfall of the
# dense log_lh at the parameters reached: 10 x the one measured on the device.  Measured: -5.9e-12 -- both runs end at
# (2.0279363, 0.6524262, 0.1017009), log_lh 139.172566, and agree beyond the dense value's own accuracy -- so 10 x its size; the
# test adds the dense values' own tolerance (1e-10 relative each, smoke()'s) on top.
OPT_SHORTFALL = 6e-11


def pcg_record(A, B, R, s, tol=TOL, maxiter=MAXITER):
    """tests/_cg_helpers.pcg (the device's freezing rule), with whole-batch products, that also records what the device
    records: alpha, beta (maxiter, S), rho0 (S,), Zt (S, n); X, iterations, relres as there."""
    B = np.atleast_2d(np.asarray(B, dtype=np.float64))
    S, n = B.shape
    X, r = np.zeros((S, n)), B.copy()
    bb = (B * B).sum(axis=1)
    rr = bb.copy()
    frozen = bb == 0.0
    iters = np.zeros(S, dtype=np.int64)
    alphas, betas = np.zeros((maxiter, S)), np.zeros((maxiter, S))
    z = woodbury(R, s, r)
    Zt = z.copy()
    rho = (r * z).sum(axis=1)
    rho0 = rho.copy()
    p = z.copy()
    it = 0
    while it < maxiter and not frozen.all():
        it += 1
        q = p @ A
        delta = (p * q).sum(axis=1)
        bad = ~frozen & ~((delta > 0.0) & np.isfinite(delta))
        frozen = frozen | bad
        iters[bad] = -it
        live = ~frozen
        alpha = np.zeros(S)
        alpha[live] = rho[live] / delta[live]
        alphas[it - 1] = alpha
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
        betas[it - 1] = beta
        rho[live] = rho_new[live]
        p[live] = z[live] + beta[live, None] * p[live]
    iters[~frozen] = it
    relres = np.where(bb > 0.0, np.sqrt(rr / np.where(bb > 0.0, bb, 1.0)), 0.0)
    return dict(X=X, iterations=iters, relres=relres, alpha=alphas, beta=betas, rho0=rho0, Zt=Zt, its=it)


def quadrature(alpha, beta):
    """e1^T log(T) e1 from the m step lengths and the first m - 1 ratios of one column; m = 0: 0."""
    a = np.asarray(alpha, dtype=np.float64)
    m = a.size
    if m == 0:
        return 0.0
    b = np.asarray(beta, dtype=np.float64)[:m - 1]
    T = np.diag(1.0 / a)
    T[np.arange(1, m), np.arange(1, m)] += b / a[:-1]
    off = np.sqrt(b) / a[:-1]
    T[np.arange(m - 1), np.arange(1, m)] = off
    T[np.arange(1, m), np.arange(m - 1)] = off
    w, v = np.linalg.eigh(T)
    return float(np.sum(v[0] ** 2 * np.log(w)))


def probe_terms_from_record(rec):
    """rho0_t e1^T log(T_t) e1 for every column of a pcg_record (or of the device's coefficient block, coef (T, maxiter, 2))."""
    its = np.abs(rec["iterations"])
    return np.array([rec["rho0"][t] * quadrature(rec["alpha"][:its[t], t], rec["beta"][:its[t], t]) for t in range(its.size)])


def logdet_precond(R, s, n):
    """log det (R^T R + s^2 I) = log det (s^2 I_k + R R^T) + (n - k) log s^2; 0 without R (P = I)."""
    k = R.shape[0]
    if k == 0:
        return 0.0
    return float(np.linalg.slogdet(s * s * np.eye(k) + R @ R.T)[1] + (n - k) * np.log(s * s))


def estimate(A, Z, R, s, tol=TOL, maxiter=MAXITER):
    """(log det estimate, per-probe terms, record) of the restatement for the probes Z (rows)."""
    rec = pcg_record(A, Z, R, s, tol, maxiter)
    terms = probe_terms_from_record(rec)
    return logdet_precond(R, s, A.shape[0]) + float(terms.mean()), terms, rec


_P, _M = {}, {}


def sqrt_pair(R, s, n):
    """(P, P^1/2, P^-1/2) of P = R^T R + s^2 I; R with no rows: three identities (P = I)."""
    if R.shape[0] == 0:
        eye = np.eye(n)
        return eye, eye, eye
    P = R.T @ R + s * s * np.eye(n)
    w, V = np.linalg.eigh(P)
    return P, (V * np.sqrt(w)) @ V.T, (V / np.sqrt(w)) @ V.T


def log_of_whitened(A, Pmh):
    """log(P^-1/2 A P^-1/2), dense and symmetric."""
    M = Pmh @ A @ Pmh
    w, V = np.linalg.eigh(0.5 * (M + M.T))
    return (V * np.log(w)) @ V.T


def precond_matrix(name, rank):
    """sqrt_pair of a problem at a rank with the restatement's R, one evaluation per (problem, rank)."""
    key = (name, rank)
    if key not in _P:
        _P[key] = sqrt_pair(reference(name, rank)["R"], PROBLEMS[name][4], PROBLEMS[name][1])
    return _P[key]


def log_whitened(name, rank):
    key = (name, rank)
    if key not in _M:
        _M[key] = log_of_whitened(reference(name, rank)["A"], precond_matrix(name, rank)[2])
    return _M[key]


def terms_of(Z, Pmh, logM):
    """The dense per-probe values u_t^T log(P^-1/2 (K + s^2 I) P^-1/2) u_t, u_t = P^-1/2 z_t."""
    U = np.atleast_2d(Z) @ Pmh
    return np.einsum("ti,ij,tj->t", U, logM, U)


def probe_terms(name, rank, Z):
    return terms_of(Z, precond_matrix(name, rank)[2], log_whitened(name, rank))


def logdet(name):
    return float(np.linalg.slogdet(reference(name, 0)["A"])[1])


def exact_probes(name, rank):
    """sqrt(n) P^1/2: T = n probes whose second moment Z^T Z / T is exactly P (rank 0: sqrt(n) I)."""
    return np.sqrt(PROBLEMS[name][1]) * precond_matrix(name, rank)[1]


def given_probes(name):
    """T_GIVEN fixed standard normal rows from numpy (the caller answers for their distribution: the per-probe terms are compared)."""
    return np.random.RandomState(500 + ord(name)).randn(T_GIVEN, PROBLEMS[name][1])


def kernel_derivatives(kind, params, x):
    """The dense derivative matrices dK/dtheta_p of K(x, x), one per kernel parameter, stacked."""
    if kind != "ard":
        okind, op, xv = oracle_view(kind, params, x)
        return orc.jacobian(okind, xv, xv, op)
    h, w = params[0], np.asarray(params[1:], dtype=np.float64)
    xs = np.asarray(x, dtype=np.float64).reshape(-1, w.size) / w
    K = orc.kernel_matrix("gaussian", "K", xs, xs, iso_params(h, w))
    t2 = (xs[:, None, :] - xs[None, :, :]) ** 2                      # (n, n, d)
    return np.stack([2.0 * K / h] + [K * (t2[:, :, k] - 1.0 / w.size) / w[k] for k in range(w.size)])


def lowrank_sums(kind, params, x, U, V):
    """(sums, mags) in the reduction's slots for c = U^T V: [P0, P1, P2, last] (Gaussian: P2 = 0; periodic), or for the ARD
    family [S_0, S_1 .. S_d, last] with S_0 = sum c k, S_k = sum c k t_k^2 on the scaled points.  mags: the same sums of
    absolute values (last: sum |U[t, j] V[t, j]|)."""
    C = U.T @ V
    Cabs = np.abs(U).T @ np.abs(V)                                   # (the bound's scale: the dot's terms taken in magnitude)
    last, last_mag = float(np.trace(C)), float(np.trace(Cabs))
    if kind == "ard":
        h, w = params[0], np.asarray(params[1:], dtype=np.float64)
        xs = np.asarray(x, dtype=np.float64).reshape(-1, w.size) / w
        K = orc.kernel_matrix("gaussian", "K", xs, xs, iso_params(h, w))
        t2 = (xs[:, None, :] - xs[None, :, :]) ** 2
        sums = [np.sum(C * K)] + [np.sum(C * K * t2[:, :, k]) for k in range(w.size)] + [last]
        mags = [np.sum(Cabs * K)] + [np.sum(Cabs * K * t2[:, :, k]) for k in range(w.size)] + [last_mag]
        return np.array(sums), np.array(mags)
    J = kernel_derivatives(kind, params, x)
    sums, mags = np.zeros(4), np.zeros(4)
    for p in range(J.shape[0]):
        sums[p], mags[p] = np.sum(C * J[p]), np.sum(Cabs * np.abs(J[p]))
    sums[3], mags[3] = last, last_mag
    return sums, mags


def dense_grad(name):
    """(gradient over (kernel parameters ..., s), the sums of the terms' magnitudes): 1/2 tr((alpha alpha^T - Ainv) dK_p),
    A = K + s^2 I, dA/ds = 2 s I."""
    kind, n, _, params, s, _ = PROBLEMS[name]
    x, y, _ = data(name)
    A = reference(name, 0)["A"]
    Ainv = np.linalg.inv(A)
    alpha = Ainv @ y
    G = np.outer(alpha, alpha) - Ainv
    J = list(kernel_derivatives(kind, params, x)) + [2.0 * s * np.eye(n)]
    return np.array([0.5 * np.sum(G * Jp) for Jp in J]), np.array([0.5 * np.sum(np.abs(G * Jp)) for Jp in J])


def grad_restated(name, rank, Z):
    """The restatement's gradient estimate for the probes Z: 1/2 alpha^T dK alpha - 1/2 (1/T) sum_t w_t^T dK zt_t."""
    kind, n, _, params, s, _ = PROBLEMS[name]
    x, y, _ = data(name)
    ref = reference(name, rank)
    rec = pcg_record(ref["A"], Z, ref["R"], s)
    alpha = ref["X"][0]
    G = np.outer(alpha, alpha) - rec["X"].T @ rec["Zt"] / Z.shape[0]
    J = list(kernel_derivatives(kind, params, x)) + [2.0 * s * np.eye(n)]
    return np.array([0.5 * np.sum(G * Jp) for Jp in J])
