"""Shared pieces of the GP.sample_paths tests: the numpy restatement of the definition in include/gpx.h ("posterior paths")
on top of `randn_ref` (tests/_sample_helpers.py, pinned to the Random123 known answers in tests/test_sample_cpu.py).

    Omega[f, k] = z(seed, 1, f d + k) / w_v      Theta[s, q] = z(seed, 2, s 2F + q)      E[s, j] = z(seed, 3, s n + j)
    phi(a) = sqrt(k0 / F) [cos(Omega a); sin(Omega a)]            k0 = h_v^2 / (w_v sqrt(2 pi))
    r_s = Phi(x) Theta_s + sigma E_s      V_s = alpha - Kxx^-1 r_s      f_s(a) = phi(a) . Theta_s + sum_j k(a, x_j) V[s, j]

on the view of the GP: the points x and (h_v, w_v) = (h, w) for the Gaussian kernel, x / w and (h / sqrt(wbar), 1) for ARD.
Everything is float64; what the device STORES in its own dtype (the points, the scaled points, Theta) is rounded through
that dtype first, as the definition says ("the point as stored in the handle's dtype")."""
import numpy as np

import gaussian_processes_amd as gp
from _ard_helpers import MIN_LOG, iso_params
from _sample_helpers import C_COND, randn_ref

_NP = {"float64": np.float64, "float32": np.float32}


def stored(a, dtype):
    """`a` as the device holds it in `dtype`, as float64."""
    return np.asarray(a, dtype=np.float64).astype(_NP[dtype]).astype(np.float64)


def view(K, pts, dtype="float64"):
    """(points (m, d) of the view, h_v, w_v) for kernel object K: the stored points, for ARD divided by the widths in `dtype`."""
    T = _NP[dtype]
    if isinstance(K, gp.GaussianARDKernel):
        w = np.asarray(K.w, dtype=np.float64)
        p = np.asarray(pts, dtype=np.float64).reshape(-1, w.size).astype(T) / w.astype(T)      # gpx_d_scale_points: a division in dtype
        h_v, w_v = iso_params(float(K.h), w)
        return p.astype(np.float64), float(h_v), float(w_v)
    p = np.asarray(pts, dtype=np.float64)
    p = p.reshape(-1, 1) if p.ndim == 1 else p
    return stored(p, dtype), float(K.h), float(K.w)


def prior_var(h_v, w_v):
    return h_v * h_v / (w_v * np.sqrt(2.0 * np.pi))


def kernel_ref(a, b, h_v, w_v):
    """k(a_i, b_j) of the isotropic Gaussian kernel on view points, with the underflow clamp."""
    e = -0.5 * ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1) / (w_v * w_v)
    return np.where(e < MIN_LOG, 0.0, prior_var(h_v, w_v) * np.exp(e))


def omega_ref(seed, F, d, w_v):
    return randn_ref(F, d, seed, stream=1) / w_v


def theta_ref(seed, S, F):
    return randn_ref(S, 2 * F, seed, stream=2)


def noise_ref(seed, S, n):
    return randn_ref(S, n, seed, stream=3)


def features_ref(pts, omega, scale):
    """(m, 2F): scale [cos(pts Omega^T), sin(pts Omega^T)]."""
    t = np.asarray(pts, dtype=np.float64) @ np.asarray(omega, dtype=np.float64).T
    return np.hstack([scale * np.cos(t), scale * np.sin(t)])


def paths_ref(g, S, F, seed, xo=None, dtype="float64"):
    """(V (S, n), f(xo) (S, m) or None, info) for GP object g in float64; info: a dict with Kxx, its condition number, alpha, r,
    the two scales of the project's bound C_COND cond(Kxx) eps scale -- scale_V = max|alpha| + max|Kxx^-1 r|,
    scale_f = max_s,i sum_q |phi_q(xo_i) Theta_sq| + max_i sum_j |k(xo_i, x_j)| scale_V (the prior term's own size, and the
    error of V carried through k(xo, x)) -- and the pieces."""
    p, h_v, w_v = view(g.K, g.x, dtype)
    n, d = p.shape
    k0 = prior_var(h_v, w_v)
    scale = np.sqrt(k0 / F)
    omega, theta, E = omega_ref(seed, F, d, w_v), stored(theta_ref(seed, S, F), dtype), noise_ref(seed, S, n)
    Kxx = kernel_ref(p, p, h_v, w_v) + float(g.s) ** 2 * np.eye(n)
    alpha = np.linalg.solve(Kxx, np.asarray(g.y, dtype=np.float64))
    Phi = features_ref(p, omega, scale)
    r = theta @ Phi.T + float(g.s) * E
    Kir = np.linalg.solve(Kxx, r.T).T if S else np.zeros((0, n))
    V = alpha - Kir
    info = dict(Kxx=Kxx, cond=float(np.linalg.cond(Kxx)), alpha=alpha, r=r, omega=omega, theta=theta, E=E, Phi=Phi, scale=scale,
                scale_V=float(np.abs(alpha).max()) + (float(np.abs(Kir).max()) if S else 0.0), view=(p, h_v, w_v))
    if xo is None:
        return V, None, info
    q, _, _ = view(g.K, xo, dtype)
    phi_o, Ko = features_ref(q, omega, scale), kernel_ref(q, p, h_v, w_v)
    f = theta @ phi_o.T + V @ Ko.T
    info["scale_f"] = (float((np.abs(theta) @ np.abs(phi_o).T).max()) + float(np.abs(Ko).sum(axis=1).max()) * info["scale_V"]
                       if S and q.shape[0] else 0.0)
    info["Ko"], info["phi_o"] = Ko, phi_o
    return V, f, info


def cond_bound(info, dtype, which):
    """The project's conditioning bound for V (which="V") or f (which="f")."""
    eps = float(np.finfo(_NP[dtype]).eps)
    return C_COND * info["cond"] * eps * info["scale_" + which]
