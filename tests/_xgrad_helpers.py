"""numpy closed forms of the input-space gradients of the predictive mean and variance, from the oracle's pieces -- the
yardstick of tests/test_gpu_xgrad.py, itself anchored against central differences of the oracle's own `mean` / `cov` in
tests/test_xgrad_cpu.py.

    gaussian  dk/da_k = -(a_k - b_k) / w^2 k                  (exactly 0 where the oracle's clamp makes k exactly 0)
    ARD       the gaussian on a / w, b / w with (h / sqrt(wbar), 1); column k divided by w_k
    periodic  dk/da_k = -sin((a_k - b_k) / p) / (p w^2) k
    dmean_i/dxo_i = sum_j alpha_j dk(xo_i, x_j)/dxo_i          alpha = Kxx^-1 y
    dvar_i/dxo_i  = -2 sum_j beta_ij dk(xo_i, x_j)/dxo_i       beta_i = Kxx^-1 k(x, xo_i)   (cho_solve with Lxx)
"""
import numpy as np
from scipy.linalg import cho_solve

from oracle import gp_oracle as orc
from _ard_helpers import ard_K


def _2d(x, d=None):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(-1, 1) if x.ndim == 1 else x


def dK_dxo(kind, params, xo, x, Kxox):
    """dK[i, j, k] = dk(xo_i, x_j)/dxo_ik from the kernel values Kxox (m, n) themselves."""
    a, b = _2d(xo), _2d(x)
    diff = a[:, None, :] - b[None, :, :]
    if kind == "gaussian":
        h, w = params
        return -(diff / (w * w)) * Kxox[:, :, None]
    if kind == "periodic":
        h, w, p = params
        return -(np.sin(diff / p) / (p * w * w)) * Kxox[:, :, None]
    if kind == "ard":
        w = np.asarray(params[1:], dtype=np.float64)
        return -(diff / (w * w)) * Kxox[:, :, None]
    raise ValueError(kind)


class RefGP(object):
    """The oracle's GP for the three families (ARD through _ard_helpers.ard_K), with the two closed-form gradients."""

    def __init__(self, kind, params, x, y, s):
        self.kind, self.params, self.s = kind, tuple(float(v) for v in params), float(s)
        self.x, self.y = _2d(x), np.asarray(y, dtype=np.float64)
        if kind == "ard":
            from scipy.linalg import cholesky
            K = ard_K(self.x, self.x, self.params[0], self.params[1:]) + self.s ** 2 * np.eye(self.x.shape[0])
            self.Lxx = cholesky(K, lower=True)
            self.alpha = cho_solve((self.Lxx, True), self.y)
        else:
            self.o = orc.OracleGP(kind, self.params, self.x, self.y, self.s)
            self.Lxx, self.alpha = self.o.Lxx, self.o.inv_Kxx_y

    def Kxox(self, xo):
        if self.kind == "ard":
            return ard_K(_2d(xo), self.x, self.params[0], self.params[1:])
        return self.o.Kxox(_2d(xo))

    def kdiag(self, xo):
        xo = _2d(xo)
        if self.kind == "ard":
            return np.array([ard_K(r[None], r[None], self.params[0], self.params[1:])[0, 0] for r in xo])
        return np.array([self.o.K(r[None], r[None])[0, 0] for r in xo])

    def mean(self, xo):
        return self.Kxox(xo) @ self.alpha

    def var(self, xo):
        K = self.Kxox(xo)
        return self.kdiag(xo) - np.einsum("ij,ij->i", K, cho_solve((self.Lxx, True), K.T).T)

    def grads(self, xo):
        """(dmean_dx, dvar_dx), each (m, d)."""
        K = self.Kxox(xo)
        dK = dK_dxo(self.kind, self.params, xo, self.x, K)
        beta = cho_solve((self.Lxx, True), K.T).T
        return np.einsum("ijk,j->ik", dK, self.alpha), -2.0 * np.einsum("ijk,ij->ik", dK, beta)


def central_differences(f, xo, step=1e-5):
    """d f(xo)_i / d xo_ik by central differences, (m, d); f maps (m, d) points to (m,) values."""
    xo = _2d(xo)
    out = np.empty(xo.shape)
    for k in range(xo.shape[1]):
        e = np.zeros(xo.shape[1])
        e[k] = step
        out[:, k] = (f(xo + e) - f(xo - e)) / (2.0 * step)
    return out
