"""Shared pieces of the tests of SparseGP's gradient: the closed form of d elbo / d (kernel parameters..., s) in dense numpy,
z held fixed and the jitter held at the value given, in the notation of tests/_sparse_helpers.py plus

    Sigma = Kuu + Phi / s^2 = Luu B Luu^T        w = Sigma^-1 b / s^2 = Luu^-T LB^-T c / s
    T  = Kuu^-1 - Sigma^-1 - w w^T               Gu = T / 2 - Kuu^-1 Phi Kuu^-1 / (2 s^2)        Gf = (T K(z, x) + w y^T) / s^2
    d elbo / d theta_p = sum Gu o dKuu/dtheta_p + sum Gf o dK(z, x)/dtheta_p - N dk(0)/dtheta_p / (2 s^2)
    d elbo / d s       = -N / s + y.y / s^3 - 2 w.b / s^3 + (N k(0) - tr X) / s^3 + tr((Sigma^-1 + w w^T) Phi) / s^3

The inverses come from the factors as the device forms them (Kuu^-1 = Luu^-T Luu^-1, Sigma^-1 = (LB^-1 Luu^-1)^T (LB^-1
Luu^-1)), so the float32 run of this restatement carries the rounding of that route and E32G is the floor it sets.
tests/test_sparse_grad_cpu.py pins the closed form against central differences of sgpr_reference's bound;
tests/test_gpu_sparse_grad.py leans on it.  Kernel derivatives: the oracle's Jacobian on the two point sets for the Gaussian
and periodic families, a rectangular numpy form in the convention of tests/_ard_helpers.py for the ARD family."""
import numpy as np
from scipy.linalg import solve_triangular

import gaussian_processes_amd as gp
from oracle import gp_oracle as orc
from _sparse_helpers import S_NOISE, auto_jitter, case_data, kernel_params, oracle_view, sgpr_reference

# (N, M) at the edges of the 64-tile and of a 128-column chunk; z = x where M == N
EDGE_PAIRS = [(1, 1), (64, 63), (65, 64), (129, 65), (300, 129)]


def _rect_derivatives(kind, params, a, b):
    """The kernel-parameter derivatives of K(a, b), one (len(a), len(b)) float64 matrix at a time, in the order of `params`."""
    if kind != "ard":
        for dK in orc.jacobian(kind, np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), tuple(params)):
            yield dK
        return
    h, w = float(params[0]), np.asarray(params[1:], dtype=np.float64)
    okind, op, av, bv = oracle_view(kind, params, a, b)
    K = orc.kernel_matrix(okind, "K", av, bv, op)
    yield 2.0 * K / h
    for k in range(w.size):
        t2 = (av[:, None, k] - bv[None, :, k]) ** 2
        yield K * (t2 / w[k] - 1.0 / (w.size * w[k]))


def sgpr_grad_reference(kind, params, x, y, z, s, jitter, dtype=np.float64):
    """(grad, scale), float64 arrays of len(params) + 1 in the order (kernel parameters..., s), every matrix in `dtype`.
    scale_p = sum |Gu| |dKuu/dtheta_p| + sum |Gf| |dK(z, x)/dtheta_p|; for s the sum of the absolute terms."""
    T = dtype
    r = sgpr_reference(kind, params, x, y, z, s, jitter, dtype)
    okind, op, xv, zv = oracle_view(kind, params, x, z)
    yv, sT = np.asarray(y, dtype=T), T(s)
    s2 = sT * sT
    N, M = xv.shape[0], zv.shape[0]
    Luu, LB, c, b = r["Luu"], r["LB"], r["c"], r["b"]
    Kzx = orc.kernel_matrix(okind, "K", zv, xv, op).astype(T)
    Phi = Kzx @ Kzx.T
    Li = solve_triangular(Luu, np.eye(M, dtype=T), lower=True)            # Luu^-1
    Kinv = Li.T @ Li
    LBi = solve_triangular(LB, Li, lower=True)                            # LB^-1 Luu^-1
    Sinv = LBi.T @ LBi
    w = solve_triangular(Luu, solve_triangular(LB, c, lower=True, trans="T"), lower=True, trans="T") / sT
    X = Li @ Phi @ Li.T
    Tm = Kinv - Sinv - np.outer(w, w)
    Gu = T(0.5) * Tm - (Li.T @ X @ Li) / (T(2.0) * s2)
    Gf = (Tm @ Kzx + np.outer(w, yv)) / s2
    z0 = np.asarray(z, dtype=np.float64)[:1]
    grad, scale = [], []
    for dKuu, dKzx, dk0 in zip(_rect_derivatives(kind, params, z, z), _rect_derivatives(kind, params, z, x),
                               _rect_derivatives(kind, params, z0, z0)):
        dKuu, dKzx, dk0 = dKuu.astype(T), dKzx.astype(T), T(dk0[0, 0])
        grad.append((Gu * dKuu).sum() + (Gf * dKzx).sum() - T(N) * dk0 / (T(2.0) * s2))
        scale.append((np.abs(Gu) * np.abs(dKuu)).sum() + (np.abs(Gf) * np.abs(dKzx)).sum())
    k0 = T(orc.kernel_matrix(okind, "K", zv[:1], zv[:1], op)[0, 0])
    s3 = s2 * sT
    terms = [-T(N) / sT, (yv @ yv) / s3, T(-2.0) * (w @ b) / s3, (T(N) * k0 - np.trace(X)) / s3,
             ((Sinv + np.outer(w, w)) * Phi).sum() / s3]
    grad.append(sum(terms[1:], terms[0]))
    scale.append(sum(abs(t) for t in terms))
    return np.array(grad, dtype=np.float64), np.array(scale, dtype=np.float64)


# ---- the data of the edge shapes and the references of every GPU case, one evaluation each --------------------------------------
# The ARD shapes beyond d = 3, one per rung of the kernel's DMAX ladder above the first (d = 9, 17, 33: DMAX = 16, 32, 64): the
# widths of test_gpu_ard._widths(d) stretched by c(d).  Unstretched, the inputs (standard deviation ~ 5.8) put the median of
# k(x_j, z_i) / k(0) over the rectangle at 1e-138 (d = 9): only coincident points would contribute, and there t_k = 0, so the S_k
# sums would be exactly zero whatever the kernel computes.  tests/test_sparse_grad_cpu.py holds the median above 1e-5.
ARD_STRETCH = {9: 6.0, 17: 8.0, 33: 12.0}
ARD_RUNG_KEYS = [("ard", 129, d, 65) for d in sorted(ARD_STRETCH)]


def edge_params(kind, d):
    if kind == "ard" and d != 3:
        from test_gpu_ard import _widths
        return (1.0,) + tuple(ARD_STRETCH[d] * _widths(d))
    return kernel_params(kind, d)


def median_kernel_ratio(key):
    """The median over the rectangle of k(x_j, z_i) / k(0) of a key."""
    params, x, _, z = problem(key)
    okind, op, xv, zv = oracle_view(key[0], params, x, z)
    K = orc.kernel_matrix(okind, "K", xv, zv, op)
    return float(np.median(K) / orc.kernel_matrix(okind, "K", zv[:1], zv[:1], op)[0, 0])


def make_kernel(kind, params):
    if kind == "gaussian":
        return gp.GaussianKernel(*params)
    if kind == "periodic":
        return gp.PeriodicKernel(*params)
    return gp.GaussianARDKernel(params[0], list(params[1:]))


_EDGE = {}


def edge_data(kind, N, d, M):
    """(kernel parameters, x, y, z) of an edge shape: the synthetic inputs of the cases, z = subset_inducing(x, M, seed=3)."""
    key = (kind, N, d, M)
    if key not in _EDGE:
        X, y, _ = orc.synth_inputs(N, d, 1)
        if d == 1:
            X = X.ravel()
        z = X.copy() if M == N else gp.SparseGP.subset_inducing(X, M, seed=3)
        for a in (X, y, z):
            a.flags.writeable = False
        _EDGE[key] = (edge_params(kind, d), X, y, z)
    return _EDGE[key]


def problem(key):
    """(kernel parameters, x, y, z) of a key (kind, N, d, M): a case of _sparse_helpers.CASES or an edge shape."""
    from _sparse_helpers import CASES
    if key in CASES:
        return case_data(key)[:4]
    return edge_data(*key)


def fp32_jitter(key):
    return auto_jitter(key[0], problem(key)[0], np.float32)


_GREF = {}


def grad_reference(key, jitter, dtype=np.float64):
    """(grad, scale, cond(Kuu)) of a key, one evaluation per (key, jitter, dtype)."""
    k = (key, float(jitter), np.dtype(dtype).name)
    if k not in _GREF:
        params, x, y, z = problem(key)
        g, sc = sgpr_grad_reference(key[0], params, x, y, z, S_NOISE, jitter, dtype)
        Kuu = sgpr_reference(key[0], params, x, y, z, S_NOISE, jitter, np.float64)["Kuu"]
        _GREF[k] = (g, sc, float(np.linalg.cond(Kuu)))
    return _GREF[k]


class _E32G(dict):
    """E32G[key]: |fp32 restatement - fp64 restatement| of the gradient, per component, both at the key's fp32 jitter."""

    def __missing__(self, key):
        jit = fp32_jitter(key)
        self[key] = np.abs(grad_reference(key, jit, np.float32)[0] - grad_reference(key, jit, np.float64)[0])
        return self[key]


E32G = _E32G()
