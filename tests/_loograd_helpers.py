"""Shared by tests/test_loograd_cpu.py and tests/test_gpu_loograd.py: the gradient of the leave-one-out criterion in numpy,
from the explicit inverse.  With W = K^-1, alpha = W y, k = diag W:

    L      = sum_i ( log(k_i) / 2 - alpha_i^2 / (2 k_i) - log(2 pi) / 2 )                       (RW06 eq. 5.10 - 5.11)
    c_i    = (1 + alpha_i^2 / k_i) / (2 k_i),   r = W (alpha / k),   P = W diag(c) W
    G      = (r alpha^T + alpha r^T) / 2 - P,   dL/dtheta_j = sum_ab dK_j,ab G_ab               (the form the device runs)
    dL/dtheta_j = sum_i ( alpha_i (Z_j alpha)_i - (1 + alpha_i^2 / k_i) (Z_j W)_ii / 2 ) / k_i,  Z_j = W dK_j    (eq. 5.13)

`dKs` is any iterable of (n, n) matrices dK/dtheta_j, the noise's 2 s I included where the caller wants it."""
import numpy as np

HALF_LOG_2PI = 0.5 * np.log(2 * np.pi)


def loo_value(K, y):
    W = np.linalg.inv(np.asarray(K, dtype=np.float64))
    a, k = W.dot(y), np.diag(W)
    return float(np.sum(0.5 * np.log(k) - 0.5 * a * a / k - HALF_LOG_2PI))


def loo_grad_from_inverse(W, alpha, dKs):
    """(value, gradient, G, scale) from W = K^-1 and alpha = K^-1 y.  scale_j = sum_ab |dK_j,ab| (|r_a alpha_b| / 2 +
    |alpha_a r_b| / 2 + (|W| diag(c) |W|)_ab): the sum of the absolute values of the terms that enter component j."""
    W, a = np.asarray(W, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    k = np.diag(W).copy()
    value = float(np.sum(0.5 * np.log(k) - 0.5 * a * a / k - HALF_LOG_2PI))
    c = 0.5 * (1.0 + a * a / k) / k
    r = W.dot(a / k)
    ra = np.outer(r, a)
    G = 0.5 * (ra + ra.T) - (W * c).dot(W)
    Gabs = 0.5 * (np.abs(ra) + np.abs(ra.T)) + (np.abs(W) * c).dot(np.abs(W))
    grad, scale = [], []
    for dK in dKs:
        grad.append(float((dK * G).sum()))
        scale.append(float((np.abs(dK) * Gabs).sum()))
    return value, np.array(grad), G, np.array(scale)


def loo_grad_reference(K, dKs, y):
    """(value, gradient, G, scale) of the GP with covariance K = K(x, x) + s^2 I and observations y, by the G form."""
    W = np.linalg.inv(np.asarray(K, dtype=np.float64))
    return loo_grad_from_inverse(W, W.dot(np.asarray(y, dtype=np.float64)), dKs)


def loo_grad_rw513(K, dKs, y):
    """The gradient by RW06 eq. 5.13 as printed: one product W dK_j per parameter."""
    W = np.linalg.inv(np.asarray(K, dtype=np.float64))
    a = W.dot(np.asarray(y, dtype=np.float64))
    k = np.diag(W)
    out = []
    for dK in dKs:
        Z = W.dot(dK)
        out.append(float(np.sum((a * Z.dot(a) - 0.5 * (1.0 + a * a / k) * np.einsum("ij,ji->i", Z, W)) / k)))
    return np.array(out)


def with_noise(J, s):
    """The kernel's Jacobian (n_kernel_params, n, n) followed by dK/ds = 2 s I: a generator, one matrix at a time."""
    n = None
    for dK in J:
        n = dK.shape[0]
        yield dK
    yield 2.0 * s * np.eye(n)
