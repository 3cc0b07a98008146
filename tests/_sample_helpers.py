"""Shared pieces of the GP.sample tests: a numpy restatement of the device generator's definition (include/gpx.h,
gpx_d_randn) -- Philox4x32-10 in uint64 arithmetic, the two uniforms, Box-Muller -- vectorised over the element index.
tests/test_sample_cpu.py pins it to the Random123 known answers; everything on the GPU is then pinned to it."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)

C_COND = 16.0                                           # tests/test_gpu_parity.py


def philox4x32_10(counter, key):
    """Philox4x32-10 of Random123.  counter: four arrays (or scalars) of 32-bit words, key: two; returns four uint64 arrays
    that hold 32-bit words."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK32 for c in counter)
    k0, k1 = (np.atleast_1d(np.asarray(k, dtype=np.uint64)) & MASK32 for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _32) ^ c1 ^ k0, p1 & MASK32, (p0 >> _32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def _unit(hi, lo):
    """(2 (((hi << 32) | lo) >> 12) + 1) 2^-53: an odd 53-bit integer, exact in float64."""
    x = (hi << _32) | lo
    return ((x >> np.uint64(12)) * np.uint64(2) + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def z_ref(seed, stream, e):
    """z(seed, stream, e) for an array of element indices e (uint64)."""
    e = np.atleast_1d(np.asarray(e, dtype=np.uint64))
    seed, stream = np.uint64(seed), np.uint64(stream)
    q = e >> np.uint64(1)
    w0, w1, w2, w3 = philox4x32_10((q & MASK32, q >> _32, stream & MASK32, stream >> _32), (seed & MASK32, seed >> _32))
    u1, u2 = _unit(w0, w1), _unit(w2, w3)
    r = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.where((e & np.uint64(1)) == 0, r * np.cos(ang), r * np.sin(ang))


def randn_ref(rows, cols, seed, stream=0, offset=0):
    """What gpx_d_randn writes into a rows x cols block, float64."""
    e = np.uint64(offset) + np.arange(rows * cols, dtype=np.uint64)
    return z_ref(seed, stream, e).reshape(rows, cols)


def auto_jitter(g, dtype):
    """sqrt(eps_dtype) k(0) from the kernel's closed form: what gpx_gp_sample takes for jitter < 0."""
    eps = float(np.finfo(np.float64 if dtype == "float64" else np.float32).eps)
    zero = np.zeros(1) if g.x.ndim == 1 else np.zeros((1, g.x.shape[1]))
    return float(np.sqrt(eps) * g.K.diag(zero)[0])


def reconstruction(g, xo, S, seed, dtype, noise, jitter=None, mean=None, cov=None):
    """(ref, bound) of a sample: ref = mean + Z chol(A)^T with A = cov + (jitter [+ s^2]) I and Z the restated normals;
    bound = C_COND cond(A) eps_dtype (max|mean| + max_s sum_k |Z_sk| sqrt(max diag A)).  mean / cov default to the GP's own."""
    eps = float(np.finfo(np.float64 if dtype == "float64" else np.float32).eps)
    mean = g.mean(xo) if mean is None else mean
    cov = g.cov(xo) if cov is None else cov
    m = mean.shape[0]
    if jitter is None:
        jitter = auto_jitter(g, dtype)
    A = cov + (jitter + (float(g.s) ** 2 if noise else 0.0)) * np.eye(m)
    A = np.tril(A) + np.tril(A, -1).T                    # the device reads the lower triangle
    Z = randn_ref(S, m, seed)
    ref = mean + Z @ np.linalg.cholesky(A).T
    scale = float(np.abs(mean).max()) + float(np.abs(Z).sum(axis=1).max()) * np.sqrt(float(np.diag(A).max()))
    return ref, C_COND * np.linalg.cond(A) * eps * scale
