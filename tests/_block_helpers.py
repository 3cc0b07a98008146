"""Helpers shared by the direct tests of device code (tests/test_gpu_blocks.py, tests/test_gpu_gemm.py): the dtype table, the
two NaN payloads regions are padded with, bitwise comparison, and the derived error bound.  tests/test_gpu_blocks.py's
docstring has the conventions and the derivation of the bound."""
import ctypes

import numpy as np

from gaussian_processes_amd import _lib

LD = np.longdouble
U = 2.0 ** -53
DTYPES = {"f64": (_lib.F64, np.float64, np.uint64, 2.0 ** -53), "f32": (_lib.F32, np.float32, np.uint32, 2.0 ** -24)}
# two NaNs with payloads of their own: what inputs are padded with, and what outputs are pre-filled with
_NAN_BITS = {np.float64: (0x7ff8000000a11ce5, 0x7ff80000000b0b00), np.float32: (0x7fc0a11c, 0x7fc00b0b)}


def gamma(k, u=U):
    return LD(k) * LD(u) / (LD(1) - LD(k) * LD(u))


def nan_in(npdt):
    return np.array([_NAN_BITS[npdt][0]], dtype=np.uint64 if npdt == np.float64 else np.uint32).view(npdt)[0]


def nan_out(npdt):
    return np.array([_NAN_BITS[npdt][1]], dtype=np.uint64 if npdt == np.float64 else np.uint32).view(npdt)[0]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def padded(rng, rows, n, ld, npdt, fill=None):
    """rows x ld, NaN everywhere, randn (drawn in float64, cast) in the first n columns."""
    a = np.full((rows, ld), nan_in(npdt) if fill is None else fill, dtype=npdt)
    a[:, :n] = rng.randn(rows, n)
    return a


def at(buf, elems, itemsize):
    return ctypes.c_void_p(buf.ptr.value + int(elems) * itemsize)


def round_up(v, m):
    return (v + m - 1) // m * m


class Worst(object):
    """The worst |got - ref| / (asserted bound) of a block, printed at the end of its test."""

    def __init__(self, block, dtype):
        self.block, self.dtype, self.ratio, self.where = block, dtype, 0.0, ""

    def check(self, got, ref, sum_abs, k, u_out, what, u_acc=U):
        """|got - ref| <= 4 (gamma_k sum_abs + u_out |ref|) componentwise; got must be finite.  u_acc: the unit roundoff of
        the accumulation (fp64 everywhere but in the product kernel behind schur_lower, which accumulates in T)."""
        got = np.asarray(got, dtype=np.float64)
        ref, sum_abs = np.asarray(ref, dtype=LD), np.asarray(sum_abs, dtype=LD)
        assert got.shape == ref.shape, what
        assert np.isfinite(got).all(), "%s: the result is not finite (something NaN was read)" % what
        err = np.abs(got.astype(LD) - ref)
        tol = 4 * (gamma(k, u_acc) * sum_abs + LD(u_out) * np.abs(ref))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
        r = float(np.max(ratio)) if ratio.size else 0.0
        if r > self.ratio:
            self.ratio, self.where = r, what
        assert r <= 1.0, "%s: |got - ref| / bound = %.3g (max err %.3e)" % (what, r, float(err.max()))

    def report(self):
        print("%s %s: worst |got - ref| / (4 x derived bound) = %.3g  (%s)" % (self.block, self.dtype, self.ratio, self.where))
