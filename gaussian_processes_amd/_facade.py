"""What the Python facades (`gp`, `sparse`, `paths`, `mlii`, `dist_gp`) share, each thing once: the dtype table, the table of
kernel families, the argument checks, the owner of a library handle and the members `GP` and `SparseGP` have in common.

Host plumbing only.  The library is reached as ``_lib.load()`` at the time of the call; an argument check never reaches it.
"""
import collections
import ctypes

import numpy as np

from . import _lib

DTYPE = np.float64

# ---- dtype ----
DTYPES = {"float64": _lib.F64, "f64": _lib.F64, np.float64: _lib.F64,
          "float32": _lib.F32, "f32": _lib.F32, np.float32: _lib.F32}


def dtype_id(dtype):
    """The library's id of a dtype in any accepted spelling; KeyError for anything else."""
    return DTYPES[dtype]


def dtype_name(dtype_id):
    return "float64" if dtype_id == _lib.F64 else "float32"


def dtype_eps(dtype_id):
    return np.finfo(np.float64 if dtype_id == _lib.F64 else np.float32).eps


# ---- kernel families ----
#: name: as `mlii` spells it; cls: the class in `.kernels`; nparams(d): kernel parameters at d input dimensions; grad_any_d: the
#: device code of the parameter derivatives covers d > 1 (else d == 1 only); hessian: the device Hessian and dm_dtheta exist;
#: paths: posterior paths (a spectral density); multi_gpu: the multi-GPU fit knows the family
Family = collections.namedtuple("Family", "name cls nparams grad_any_d hessian paths multi_gpu")
FAMILIES = {
    _lib.KERNEL_GAUSSIAN: Family("gaussian", "GaussianKernel", lambda d: 2, True, True, True, True),
    _lib.KERNEL_PERIODIC: Family("periodic", "PeriodicKernel", lambda d: 3, False, True, False, True),
    _lib.KERNEL_GAUSSIAN_ARD: Family("gaussian_ard", "GaussianARDKernel", lambda d: d + 1, True, False, True, False),
}
FAMILY_IDS = dict((f.name, kid) for kid, f in FAMILIES.items())


def kernel_class(kid):
    from . import kernels
    return getattr(kernels, FAMILIES[kid].cls)


def native_id(K, d=None):
    """The library's id of the kernel object `K`, None for a plugin kernel; with `d`, an ARD kernel must have that many widths."""
    kid = getattr(K, "_native_kernel", None)
    if d is not None and kid == _lib.KERNEL_GAUSSIAN_ARD and d != K.d:
        raise ValueError("x has %d dimension(s), the kernel has %d width(s)" % (d, K.d))
    return kid


def device_grad(kid, d):
    """Does the gradient of `log_lh` and of the LOO criterion stay on the device?"""
    return kid is not None and (d == 1 or FAMILIES[kid].grad_any_d)


def device_hessian(kid, d):
    """Do the Hessian and `dm_dtheta` stay on the device?"""
    return device_grad(kid, d) and FAMILIES[kid].hessian


def has_paths(kid):
    return kid is not None and FAMILIES[kid].paths


# ---- argument checks: the normalised value, or the refusal ----
def _is_int(val):
    return isinstance(val, (int, np.integer)) and not isinstance(val, bool)


def chunk_arg(name, val, strict=False):
    """Rows or columns per device chunk: 0 (automatic) or a multiple of 128.  `strict` refuses what is not an int (bools and
    floats too) where the default takes ``int(val)``."""
    shown = "%r" % (val,)
    if not strict:
        val = int(val)
        shown = "%d" % val
    if not _is_int(val) or val < 0 or val % 128:
        raise ValueError("invalid value for %s: %s (0, or a multiple of 128)" % (name, shown))
    return int(val)


def seed_arg(seed):
    """An int in [0, 2**64); None draws one from numpy's global state, the high half first."""
    if seed is None:
        return int(np.random.randint(0, 2 ** 32)) << 32 | int(np.random.randint(0, 2 ** 32))
    if not _is_int(seed) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("invalid value for seed: %r (None, or an int in [0, 2**64))" % (seed,))
    return int(seed)


def count_arg(name, val, minimum, none_ok=False):
    """An int >= `minimum`; None passes through where `none_ok`."""
    if val is None and none_ok:
        return None
    if not _is_int(val) or val < minimum:
        raise ValueError("invalid value for %s: %r (%san int >= %d)" % (name, val, "None, or " if none_ok else "", minimum))
    return int(val)


def nonneg_float_arg(name, val, sample_wording=False):
    """None, or a finite float >= 0.  `sample_wording`: `GP.sample`'s texts -- "float" for "number", and one of their own for a
    value ``float()`` does not take, which otherwise raises what ``float()`` raises."""
    if val is None:
        return None
    try:
        val = float(val)
    except (TypeError, ValueError):
        if not sample_wording:
            raise
        raise ValueError("invalid value for %s: %r (None, or a float >= 0)" % (name, val))
    if not (val >= 0.0) or not np.isfinite(val):
        raise ValueError("invalid value for %s: %r (None, or a finite %s >= 0)" % (name, val, "float" if sample_wording else "number"))
    return val


def points_arg(name, val, d, ndim=None):
    """``(array, m)``: `val` as contiguous float64 test points ``(m,)`` (d == 1) or ``(m, d)``; with ``ndim=2`` the inputs were
    given as ``(n, d)`` and a 1-D array is refused even at d == 1."""
    arr = np.ascontiguousarray(val, dtype=DTYPE)
    if arr.ndim not in (1, 2) or (1 if arr.ndim == 1 else arr.shape[1]) != d or (arr.ndim == 1 and ndim == 2):
        raise ValueError("invalid shape for %s: %s" % (name, str(arr.shape)))
    return arr, arr.shape[0]


def check_finite(a):
    # scipy.linalg.cholesky(..., check_finite=True) (gp/gp.py:294)
    if not np.isfinite(a).all():
        raise ValueError("array must not contain infs or NaNs")


# ---- handles ----
def select_device(device):
    """Make `device` the calling host thread's current GPU (None: leave it) and return the library."""
    lib = _lib.load()
    if device is not None:
        _lib.check(lib.gpx_set_device(int(device)))
    return lib


def timing(entry, handle, names):
    """The float array of milliseconds that `entry` fills for `handle`, as a dict under `names`."""
    ms = (ctypes.c_float * len(names))()
    _lib.check(getattr(_lib.load(), entry)(handle, ms))
    return dict(zip(names, list(ms)))


class Handle(object):
    """Owner of one library handle: the pointer (in the attribute a subclass names), the entry that destroys it, `close`, and
    a `__del__` that survives interpreter shutdown."""
    _pointer = "handle"
    _destroy = None

    def __init__(self, destroy=None, ptr=None):
        if destroy is not None:
            self._destroy = destroy
        setattr(self, self._pointer, ptr if ptr is not None else ctypes.c_void_p())

    def close(self):
        if getattr(self, self._pointer, None):
            getattr(_lib.load(), self._destroy)(getattr(self, self._pointer))
            setattr(self, self._pointer, ctypes.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass


# ---- members GP and SparseGP share ----
class ParamsMixin(object):
    """``params`` and ``set_param`` of an object with a kernel `K`, a noise level `s` and `_invalidate()`."""

    @property
    def params(self):
        r"""``(kernel parameters..., s)`` (gp/gp.py:199-214)."""
        kp = self.K.params
        out = np.empty(kp.size + 1)
        out[:-1] = kp
        out[-1] = self._s
        return out

    @params.setter
    def params(self, val):
        if np.any(self.params != val):
            self._invalidate()
            self.K.params = val[:-1]
            self.s = val[-1]

    def set_param(self, name, val):
        if name == "s":
            self.s = val
            return
        if getattr(self.K, name) != val:      # AttributeError for an unknown name
            self._invalidate()
            self.K.set_param(name, val)
