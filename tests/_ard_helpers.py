"""numpy closed forms of the Gaussian ARD kernel and of the gradient of its log marginal likelihood -- the yardstick of
tests/test_gpu_ard.py, itself checked against central differences of the oracle in tests/test_ard_cpu.py.

    k(a, b) = h^2 / sqrt(2 pi wbar^2) exp(-1/2 sum_k t_k^2),  t_k = (a_k - b_k) / w_k,  wbar = (prod w_k)^(1/d)
    dk/dh = 2 k / h          dk/dw_k = k (t_k^2 / w_k - 1 / (d w_k))
    dloglh/dtheta_i = 1/2 sum_ab (alpha alpha^T - K^-1)_ab dK_i,ab          (RW06 eq. 5.9; dK/ds = 2 s I)
"""
import numpy as np

MIN_LOG = -705.6238298100243


def wbar(w):
    w = np.asarray(w, dtype=np.float64)
    return float(np.exp(np.log(w).sum() / w.size))


def iso_params(h, w):
    """The isotropic parameters that go with the scaled points x / w."""
    return (h / np.sqrt(wbar(w)), 1.0)


def ard_K(x1, x2, h, w):
    w = np.asarray(w, dtype=np.float64)
    a, b = np.asarray(x1, dtype=np.float64).reshape(-1, w.size) / w, np.asarray(x2, dtype=np.float64).reshape(-1, w.size) / w
    e = -0.5 * ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    return np.where(e < MIN_LOG, 0.0, h * h / np.sqrt(2.0 * np.pi) / wbar(w) * np.exp(e))


def ard_dK(x, h, w):
    """The d + 1 kernel-parameter derivatives of K(x, x), one (n, n) matrix at a time (a generator: never (d + 1, n, n))."""
    w = np.asarray(w, dtype=np.float64)
    xs = np.asarray(x, dtype=np.float64).reshape(-1, w.size) / w
    K = ard_K(x, x, h, w)
    yield 2.0 * K / h
    for k in range(w.size):
        t2 = (xs[:, None, k] - xs[None, :, k]) ** 2
        yield K * (t2 / w[k] - 1.0 / (w.size * w[k]))


def ard_grad(x, h, w, s, Kinv, alpha):
    """(gradient (d + 2,) in the order (h, w_1 ... w_d, s), scale (d + 2,)) from K^-1 and alpha = K^-1 y.
    scale_i = |alpha|^T |dK_i| |alpha| + sum |K^-1| o |dK_i|: the size of the terms that enter component i (the `sc1` of
    tests/test_gpu_parity.py::_check_gp_record, with this family's dK)."""
    A = np.outer(alpha, alpha) - Kinv
    aabs, Kabs = np.abs(alpha), np.abs(Kinv)
    grad, scale = [], []
    for dK in ard_dK(x, h, w):
        grad.append(0.5 * float((A * dK).sum()))
        scale.append(float(aabs @ np.abs(dK) @ aabs) + float((Kabs * np.abs(dK)).sum()))
    n = alpha.size
    grad.append(float(s * (alpha @ alpha - np.trace(Kinv))))
    scale.append(2.0 * s * (float(aabs @ aabs) + float(np.abs(np.diag(Kinv)).sum())))
    assert len(grad) == len(w) + 2 and n == Kinv.shape[0]
    return np.array(grad), np.array(scale)
