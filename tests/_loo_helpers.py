"""Shared by tests/test_loo_cpu.py and tests/test_gpu_loo.py: the closed form of leave-one-out cross-validation
(RW06 eq. 5.10 - 5.12) in numpy, from the explicit inverse."""
import numpy as np

HALF_LOG_2PI = 0.5 * np.log(2 * np.pi)


def loo_from_diag(kii, alpha, y):
    """(mean, var, log_p) per point from k = diag(K^-1), alpha = K^-1 y and y."""
    mean = y - alpha / kii
    var = 1.0 / kii
    log_p = 0.5 * np.log(kii) - 0.5 * alpha * alpha / kii - HALF_LOG_2PI
    return mean, var, log_p


def loo_reference(K, y):
    """(diag(K^-1), mean, var, log_p) of the GP with covariance K = K(x, x) + s^2 I and observations y: the prediction
    for y_i, noise included, of the GP fitted without point i, and the log density of y_i under it."""
    Ki = np.linalg.inv(np.asarray(K, dtype=np.float64))
    kii = np.diag(Ki).copy()
    return (kii,) + loo_from_diag(kii, Ki.dot(y), np.asarray(y, dtype=np.float64))
