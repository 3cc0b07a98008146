"""Shared pieces of the PosteriorPaths.grad tests: the numpy restatement of a path's input-space gradient on top of
`paths_ref` (tests/_paths_helpers.py).  On the view of the GP -- points p, constants (h_v, w_v), a = the view of xo:

    d f_s / d a_k (a) =  sqrt(k0 / F) sum_f Omega[f, k] (Theta[s, F + f] cos(Omega_f . a) - Theta[s, f] sin(Omega_f . a))
                        - 1 / w_v^2 sum_j V[s, j] (a_k - p_jk) k(a, p_j)

and for the ARD kernel component k is divided by w_k (a = xo / w).  Everything is float64; what the device stores in its own
dtype is rounded through that dtype first, as `paths_ref` does."""
import numpy as np

import gaussian_processes_amd as gp
from _paths_helpers import paths_ref, view


def col_div(K, d):
    """What component k of a gradient on the view is divided by: the ARD widths, else ones."""
    return np.asarray(K.w, dtype=np.float64) if isinstance(K, gp.GaussianARDKernel) else np.ones(d)


def features_grad_ref(pts, omega, scale, div=None):
    """(m, d, 2F): row (i, k) = d phi(p_i) / d p_ik [/ div_k] = (scale / div_k) Omega[:, k] [-sin(Omega p_i), cos(Omega p_i)]."""
    pts, omega = np.asarray(pts, dtype=np.float64), np.asarray(omega, dtype=np.float64)
    t = pts @ omega.T                                                          # (m, F)
    c = (scale / (np.ones(pts.shape[1]) if div is None else np.asarray(div, dtype=np.float64)))[:, None] * omega.T   # (d, F)
    return np.concatenate([-(c[None] * np.sin(t)[:, None, :]), c[None] * np.cos(t)[:, None, :]], axis=2)


def kernel_grad_ref(q, p, Ko, w_v, div=None):
    """(m, n, d): d k(q_i, p_j) / d q_ik [/ div_k] = -(q_ik - p_jk) / w_v^2 k(q_i, p_j)."""
    dK = -(q[:, None, :] - p[None, :, :]) / (w_v * w_v) * Ko[:, :, None]
    return dK if div is None else dK / np.asarray(div, dtype=np.float64)


def grad_ref(g, S, F, seed, xo, dtype="float64"):
    """(f (S, m), G (S, m, d), info) for GP object g in float64: `paths_ref`'s values and info, the gradient above, and
    info["scale_g"] = max_s,i,k sum_q |psi_q(xo_i)_k Theta_sq| + max_i,k sum_j |dk(xo_i, x_j)/dxo_ik| scale_V -- the analogue of
    scale_f, the ARD division by w_k included."""
    V, f, info = paths_ref(g, S, F, seed, xo=xo, dtype=dtype)
    p, h_v, w_v = info["view"]
    q = view(g.K, xo, dtype)[0]
    div = col_div(g.K, p.shape[1])
    psi = features_grad_ref(q, info["omega"], info["scale"], div)             # (m, d, 2F)
    dK = kernel_grad_ref(q, p, info["Ko"], w_v, div)                          # (m, n, d)
    G = np.einsum("sq,ikq->sik", info["theta"], psi) + np.einsum("sj,ijk->sik", V, dK)
    info["psi"], info["dK"] = psi, dK
    info["scale_g"] = (float(np.einsum("sq,ikq->sik", np.abs(info["theta"]), np.abs(psi)).max())
                       + float(np.abs(dK).sum(axis=1).max()) * info["scale_V"] if S and q.shape[0] else 0.0)
    return f, G, info
