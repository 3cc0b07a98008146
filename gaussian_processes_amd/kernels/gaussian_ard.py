"""GaussianARDKernel -- the Gaussian kernel with one length-scale per input dimension (automatic relevance
determination, RW06 eq. 5.1); an extension: the reference has no such kernel.

With ``t_k = (a_k - b_k) / w_k`` and the geometric mean ``wbar = (prod_k w_k) ** (1 / d)``

    k(a, b) = h^2 / sqrt(2 pi wbar^2) * exp(-1/2 sum_k t_k^2)

with the reference's underflow clamp (an entry whose exponent is below MIN is exactly 0).  At equal widths this is
`GaussianKernel(h, w)` on (n, d) inputs.  Parameters are ``(h, w_1 ... w_d)``; their derivatives

    dk/dh = 2 k / h        dk/dw_k = k (t_k^2 / w_k - 1 / (d w_k))

are only ever needed inside ``GP.dloglh_dtheta``, which evaluates them on the device without materialising a
(d + 1, n, n) Jacobian -- `jacobian` and `hessian` are therefore not offered.
"""
import numpy as np

from .. import _lib
from .base import Kernel
from ._native import DTYPE, member_matrix, points, positive_param, self_distance

__all__ = ["GaussianARDKernel"]


class GaussianARDKernel(Kernel):
    _native_kernel = _lib.KERNEL_GAUSSIAN_ARD

    def __init__(self, h, w):
        w = np.atleast_1d(np.asarray(w, dtype=DTYPE))
        if w.ndim != 1 or not 1 <= w.size <= _lib.ARD_MAX_D:
            raise ValueError("w must hold between 1 and %d widths, one per input dimension (got shape %s)"
                             % (_lib.ARD_MAX_D, str(w.shape)))
        self.h = None    #: output scale
        self._w = np.empty(w.size, dtype=DTYPE)
        self.params = np.concatenate([[h], w])

    @property
    def d(self):
        """Number of input dimensions (= number of widths)."""
        return self._w.size

    @property
    def w(self):
        """The d input scales, a read-only float64 array."""
        out = self._w.view()
        out.flags.writeable = False
        return out

    @property
    def _param_names(self):
        return ("h",) + tuple("w%d" % k for k in range(self.d))

    @property
    def params(self):
        """``(h, w_1 ... w_d)`` as a float64 array."""
        return np.concatenate([[self.h], self._w]).astype(DTYPE)

    @params.setter
    def params(self, val):
        val = np.asarray(val, dtype=DTYPE).ravel()
        if val.size != self.d + 1:
            raise ValueError("params must hold %d values (h, w_1 ... w_%d), got %d" % (self.d + 1, self.d, val.size))
        # every entry is checked before any is stored
        new = [positive_param(name, v) for name, v in zip(self._param_names, val)]
        self.h = new[0]
        self._w[:] = new[1:]

    def _index(self, name):
        if isinstance(name, str) and name[:1] == "w" and name[1:].isdigit() and int(name[1:]) < self.d \
                and name == "w%d" % int(name[1:]):
            return int(name[1:])
        return None

    def set_param(self, name, val):
        if name == "h":
            self.h = positive_param(name, val)
            return
        k = self._index(name)
        if k is None:
            raise ValueError("unknown parameter: %s" % name)
        self._w[k] = positive_param(name, val)

    def __getattr__(self, name):
        # only reached when normal lookup fails: "w0" ... "w{d-1}"
        if name != "_w" and "_w" in self.__dict__:
            k = self._index(name)
            if k is not None:
                return self._w[k]
        raise AttributeError("%s object has no attribute %r" % (type(self).__name__, name))

    # the base class copies with type(self)(*self.params), which does not fit (h, w)
    def __getstate__(self):
        return {"params": self.params}

    def __setstate__(self, state):
        p = np.asarray(state["params"], dtype=DTYPE)
        self.h = None
        self._w = np.empty(p.size - 1, dtype=DTYPE)
        self.params = p

    def __copy__(self):
        return type(self)(self.h, self._w)

    def __deepcopy__(self, memo):
        return type(self)(self.h, self._w.copy())

    @property
    def wbar(self):
        """Geometric mean of the widths, ``exp(sum_k log w_k / d)``."""
        return np.exp(np.log(self._w).sum() / self.d)

    def K(self, x1, x2, out=None):
        for x in (x1, x2):
            _, _, d = points(x)
            if d != self.d:
                raise ValueError("inputs have %d dimension(s), the kernel has %d width(s)" % (d, self.d))
        return member_matrix(self._native_kernel, _lib.K, self.params, x1, x2, out)

    def diag(self, x):
        r"""``k(x_i, x_i) = h^2 / sqrt(2 pi) / wbar``, ``(n,)``, in closed form."""
        return (self.h * self.h) / np.sqrt(2.0 * np.pi) / self.wbar + self_distance(x)

    def jacobian(self, x1, x2, out=None):
        raise NotImplementedError("GaussianARDKernel has no materialised Jacobian: GP.dloglh_dtheta evaluates the "
                                  "d + 1 parameter derivatives on the device")

    def hessian(self, x1, x2, out=None):
        raise NotImplementedError("GaussianARDKernel has no second parameter derivatives (GP.dloglh_dtheta is the "
                                  "derivative this family offers)")
