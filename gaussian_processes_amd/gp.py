"""GP -- drop-in for the reference's ``gp.GP`` (gp/gp.py:44-700) on MI355X.

Same constructor, properties, methods, error behaviour and memoisation rules as
the reference; the arithmetic of the hot path -- kernel-matrix build, Cholesky,
triangular solves, log-determinant, posterior mean / covariance -- runs in
hand-written HIP kernels behind the C ABI of libgpx.so.  The fitted state
(x, y, the factor, alpha) lives in HBM inside a ``gpx_gp`` handle; host copies
of the big matrices (`Kxx`, `Lxx`, `inv_Kxx`) are only made when those
properties are actually read, so `log_lh`, `inv_Kxx_y`, `mean`, `cov` work at
sizes whose n x n matrices would not fit host memory comfortably.

Extensions beyond the reference (which is strictly 1-D, float64):
  * ``x`` may be (n, d); ``y`` must then be (n,).
  * ``dtype='float32'`` runs the device path in fp32 (results are still
    returned as float64 arrays / numpy.float64 scalars).
  * ``device=k`` selects the GPU.
"""
import ctypes
import logging
from copy import copy, deepcopy

import numpy as np

from . import _lib
from ._facade import (FAMILIES, Handle, ParamsMixin, check_finite, chunk_arg, count_arg, device_grad, device_hessian,
                      dtype_eps, dtype_id, dtype_name, has_paths, kernel_class, native_id, nonneg_float_arg, points_arg, seed_arg,
                      select_device, timing)
from .ext import gp_c

__all__ = ["GP"]

logger = logging.getLogger("gp.gp")

DTYPE = np.float64
EPS = np.finfo(DTYPE).eps
MIN = np.log(np.exp2(DTYPE(np.finfo(DTYPE).minexp + 4)))   # gp/gp.py:17


def memoprop(f):
    """Memoised property: computed on first access, cached in ``self._memoized``
    under the property's name, evicted by ``del obj.prop`` (gp/gp.py:20-41)."""
    name = f.__name__

    def fget(self):
        cache = self._memoized
        if name not in cache:
            cache[name] = f(self)
        return cache[name]

    def fdel(self):
        del self._memoized[name]

    return property(fget=fget, fdel=fdel, doc=f.__doc__)


class _DeviceState(Handle):
    """Owns the gpx_gp handle of one GP; rebuilt whenever shape/dtype change.  `handle`: an existing fitted gpx_gp handle to
    wrap (gpx_gp_load, gpx_gp_extend, gpx_gp_remove) instead of a new one."""
    _destroy = "gpx_gp_destroy"

    def __init__(self, dtype_id, kernel_id, n, d, device, handle=None):
        Handle.__init__(self, ptr=handle)
        self.key = (dtype_id, kernel_id, n, d, device)
        self.data_version = self.params_version = self.fit_version = -1
        self.info = None
        if handle is None:
            _lib.check(select_device(device).gpx_gp_create(ctypes.byref(self.handle), dtype_id, kernel_id, n, d))


class GP(ParamsMixin):
    r"""Gaussian process regression object.

    Parameters
    ----------
    K : :class:`~gaussian_processes_amd.kernels.Kernel`
        Kernel object
    x : numpy.ndarray
        :math:`n` array of input locations (or ``(n, d)``)
    y : numpy.ndarray
        :math:`n` array of observations
    s : number (default=0)
        Standard deviation of the observation noise
    """

    def __init__(self, K, x, y, s=0, dtype="float64", device=None):
        self.K = K
        self._x = None
        self._y = None
        self._s = None
        self._memoized = {}
        self._dtype = dtype_id(dtype)
        self._device = device
        self._dev = None          # _DeviceState, created lazily
        self._version = 0         # bumped by every invalidation
        self._data_version = 0    # bumped when x or y change

        self.x = x
        self.y = y
        self.s = s

    # ---- state: exactly the reference's five entries (gp/gp.py:78-92) ----
    def __getstate__(self):
        state = {"K": self.K, "_x": self._x, "_y": self._y, "_s": self._s,
                 "_memoized": self._memoized}
        # the two extensions ride along only when they are in use: a GP built the reference's way
        # (float64, default device) pickles to exactly the reference's five keys
        if self._dtype != _lib.F64 or self._device is not None:
            state["_gpx"] = {"dtype": self._dtype, "device": self._device}
        return state

    def __setstate__(self, state):
        self.K = state["K"]
        self._x = state["_x"]
        self._y = state["_y"]
        self._s = state["_s"]
        self._memoized = state["_memoized"]
        extra = state.get("_gpx", {})
        self._dtype = extra.get("dtype", _lib.F64)
        self._device = extra.get("device", None)
        self._dev = None
        self._version = 0
        self._data_version = 0

    def __copy__(self):
        new = type(self).__new__(type(self))
        new.__setstate__(self.__getstate__())
        return new

    def __deepcopy__(self, memo):
        new = type(self).__new__(type(self))
        new.__setstate__(deepcopy(self.__getstate__(), memo))
        return new

    def copy(self, deep=True):
        """Deep (default) or shallow copy of the GP object."""
        return deepcopy(self) if deep else copy(self)

    # ---- invalidation ----
    def _invalidate(self, data=False):
        self._memoized = {}
        self._version += 1
        if data:
            self._data_version += 1

    # ---- inputs (gp/gp.py:129-197) ----
    @property
    def x(self):
        r"""Input locations, read-only float64 copy."""
        return self._x

    @x.setter
    def x(self, val):
        if np.any(val != self._x):
            arr = np.array(val, copy=True, dtype=DTYPE)
            if arr.ndim not in (1, 2):
                raise ValueError("invalid shape for x: %s" % str(arr.shape))
            self._invalidate(data=True)
            self._x = arr
            self._x.flags.writeable = False

    @property
    def y(self):
        r"""Observations, read-only float64 copy."""
        return self._y

    @y.setter
    def y(self, val):
        if np.any(val != self._y):
            self._invalidate(data=True)
            self._y = np.array(val, copy=True, dtype=DTYPE)
            self._y.flags.writeable = False
            expected = self._x.shape if self._x.ndim == 1 else (self._x.shape[0],)
            if self._y.shape != expected:
                raise ValueError("invalid shape for y: %s" % str(self._y.shape))

    @property
    def s(self):
        r"""Standard deviation of the observation noise (numpy.float64)."""
        return self._s

    @s.setter
    def s(self, val):
        if val < 0:
            raise ValueError("invalid value for s: %s" % val)
        if val != self._s:
            self._invalidate()
            self._s = DTYPE(val)

    def get_param(self, name):
        return self.s if name == "s" else getattr(self.K, name)

    # ---- device plumbing ----
    @property
    def _n(self):
        return self._x.shape[0]

    @property
    def _d(self):
        return 1 if self._x.ndim == 1 else self._x.shape[1]

    def _state(self):
        kid = native_id(self.K, self._d)
        key = (self._dtype, _lib.KERNEL_GAUSSIAN if kid is None else kid, self._n, self._d,
               self._device)
        if self._dev is None or self._dev.key != key:
            if self._dev is not None:
                self._dev.close()
            self._dev = _DeviceState(*key)
        st = self._dev
        if st.data_version != self._data_version:
            xs = np.ascontiguousarray(self._x, dtype=DTYPE)
            ys = np.ascontiguousarray(self._y, dtype=DTYPE)
            _lib.check(_lib.load().gpx_gp_set_data(st.handle, _lib.dptr(xs), _lib.dptr(ys)))
            st.data_version = self._data_version
            st.params_version = -1
            st.fit_version = -1
        return st

    def _sync_params(self, st):
        """Push (kernel params, s) to the handle once per invalidation."""
        if st.params_version != self._version:
            p = np.ascontiguousarray(self.K.params, dtype=DTYPE)
            _lib.check(_lib.load().gpx_gp_set_params(st.handle, _lib.dptr(p), float(self._s)))
            st.params_version = self._version
            st.fit_version = -1

    def _fit(self):
        """Make the device state current: Kxx -> Lxx -> alpha -> logdet (one pass)."""
        st = self._state()
        if st.fit_version == self._version:
            return st
        lib = _lib.load()
        if native_id(self.K) is not None:
            self._sync_params(st)
        else:
            # plugin kernel: its own Python K() on the host, matrix uploaded
            Kxx = np.ascontiguousarray(self.Kxx, dtype=DTYPE)
            check_finite(Kxx)
            _lib.check(lib.gpx_gp_set_K(st.handle, _lib.dptr(Kxx), Kxx.shape[1]))
        info = ctypes.c_int(0)
        _lib.check(lib.gpx_gp_fit(st.handle, ctypes.byref(info)))
        st.info = info.value
        st.fit_version = self._version
        return st

    def _fit_pd(self):
        st = self._fit()
        if st.info != 0:
            raise _lib.lapack_info_error(st.info)
        return st

    # ---- memoised hot-path properties ----
    @memoprop
    def Kxx(self):
        r"""Kernel covariance matrix :math:`K(x, x) + s^2 I` (gp/gp.py:242-266)."""
        if native_id(self.K) is None:
            K = self.K(self._x, self._x)
            K[np.diag_indices_from(K)] += self._s ** 2
            return K
        st = self._state()
        self._sync_params(st)
        out = np.empty((self._n, self._n), dtype=DTYPE)
        _lib.check(_lib.load().gpx_gp_get_Kxx(st.handle, _lib.dptr(out), self._n))
        return out

    @memoprop
    def Kxx_J(self):
        return self.K.jacobian(self._x, self._x)

    @memoprop
    def Kxx_H(self):
        return self.K.hessian(self._x, self._x)

    @memoprop
    def Lxx(self):
        r"""Lower Cholesky factor of `Kxx` (gp/gp.py:278-294); raises
        numpy.linalg.LinAlgError when `Kxx` is not positive definite."""
        st = self._fit_pd()
        out = np.empty((self._n, self._n), dtype=DTYPE)
        _lib.check(_lib.load().gpx_gp_get_Lxx(st.handle, _lib.dptr(out), self._n))
        return out

    @memoprop
    def inv_Kxx(self):
        r"""Explicit inverse :math:`K_{xx}^{-1} = L^{-\top} L^{-1}` (gp/gp.py:296-312)."""
        st = self._fit_pd()
        out = np.empty((self._n, self._n), dtype=DTYPE)
        _lib.check(_lib.load().gpx_gp_get_inv_Kxx(st.handle, _lib.dptr(out), self._n))
        return out

    @memoprop
    def inv_Kxx_y(self):
        r""":math:`K_{xx}^{-1} y` by forward + back substitution (gp/gp.py:314-335)."""
        st = self._fit_pd()
        out = np.empty(self._n, dtype=DTYPE)
        _lib.check(_lib.load().gpx_gp_get_alpha(st.handle, _lib.dptr(out)))
        return out

    @memoprop
    def log_lh(self):
        r"""Log marginal likelihood, RW06 eq. 5.8 (gp/gp.py:337-367, gp_c.pyx:17-31):
        ``-inf`` when `Kxx` is not positive definite or ``logdet < MIN``."""
        st = self._fit()
        if st.info != 0:
            return -np.inf
        out = ctypes.c_double(0.0)
        _lib.check(_lib.load().gpx_gp_log_lh(st.handle, ctypes.byref(out)))
        return DTYPE(out.value)

    @memoprop
    def lh(self):
        r"""Marginal likelihood ``exp(log_lh)``, 0 below ``MIN`` (gp/gp.py:369-396)."""
        llh = self.log_lh
        if llh < MIN:
            return 0
        return np.exp(llh)

    # ---- derivative stack (gp/gp.py:398-502): formulas of gp_c.pyx, products on device ----
    def _nan_or(self, shape):
        out = np.empty(shape)
        try:
            Ki = self.inv_Kxx
        except np.linalg.LinAlgError:
            out.fill(np.nan)
            return out, None
        return out, Ki

    @memoprop
    def dloglh_dtheta(self):
        r"""Gradient of the log marginal likelihood, RW06 eq. 5.9 (gp/gp.py:398-433).  Native
        kernels: computed entirely on the device (K^-1 never leaves HBM, the kernel Jacobian
        is never materialised); plugin kernels: the reference's formula with device products."""
        npar = len(self.params)
        if device_grad(native_id(self.K), self._d):
            st = self._fit()
            out = np.empty(npar, dtype=DTYPE)
            _lib.check(_lib.load().gpx_gp_dloglh_dtheta(st.handle, _lib.dptr(out)))
            return out
        out, Ki = self._nan_or(npar)
        if Ki is not None:
            gp_c.dloglh_dtheta(_c(self._y), Ki, _c(self.Kxx_J), self.inv_Kxx_y, self._s, out)
        return out

    def _native_derivs(self):
        """True when the derivative stack can stay on the device (built-in kernel; periodic: 1-D)."""
        return device_hessian(native_id(self.K), self._d)

    def _no_ard(self, name):
        kid = native_id(self.K)
        if kid is not None and not FAMILIES[kid].hessian:
            raise NotImplementedError("%s is not implemented for GaussianARDKernel (dloglh_dtheta and dlh_dtheta are)" % name)

    @memoprop
    def dlh_dtheta(self):
        r"""Gradient of the marginal likelihood (gp/gp.py:435-465).  Native kernels: device resident."""
        if device_grad(native_id(self.K), self._d):
            # gp_c.pyx:52-67 is lh times gp_c.pyx:34-49 term by term: 0.5 lh (y^T K^-1 dK K^-1 y - tr(K^-1 dK))
            return np.asarray(self.lh * self.dloglh_dtheta, dtype=DTYPE)
        out, Ki = self._nan_or(len(self.params))
        if Ki is not None:
            gp_c.dlh_dtheta(_c(self._y), Ki, _c(self.Kxx_J), self.inv_Kxx_y, self._s, self.lh, out)
        return out

    @memoprop
    def d2lh_dtheta2(self):
        r"""Hessian of the marginal likelihood (gp/gp.py:467-502).  Native kernels: device resident
        (K^-1, the K^-1 dK_i products and all traces / quadratic forms stay in HBM)."""
        self._no_ard("d2lh_dtheta2")
        if self._native_derivs():
            st = self._fit()
            npar = len(self.params)
            out = np.empty((npar, npar), dtype=DTYPE)
            hess = np.empty((npar, npar), dtype=DTYPE)
            _lib.check(_lib.load().gpx_gp_dlh_d2lh(st.handle, None, _lib.dptr(out), _lib.dptr(hess)))
            self._memoized.setdefault("d2loglh_dtheta2", hess)       # same device pass
            return out
        npar = len(self.params)
        out, Ki = self._nan_or((npar, npar))
        if Ki is not None:
            gp_c.d2lh_dtheta2(_c(self._y), Ki, _c(self.Kxx_J), _c(self.Kxx_H), self.inv_Kxx_y, self._s,
                              self.lh, _c(self.dlh_dtheta), out)
        return out

    @memoprop
    def d2loglh_dtheta2(self):
        r"""Hessian of the LOG marginal likelihood w.r.t. ``(kernel params..., s)`` -- an extension:
        the reference only offers the lh-scaled `d2lh_dtheta2`, which is identically zero once
        ``log_lh < MIN`` (any n beyond a few hundred).  ``d2lh / lh - (dlh / lh)(dlh / lh)^T`` from the
        same device pass (csrc/gpx_deriv.hip); native kernels only.  NaN when `Kxx` is not PD."""
        self._no_ard("d2loglh_dtheta2")
        if not self._native_derivs():
            raise NotImplementedError("d2loglh_dtheta2 needs a built-in kernel (periodic: 1-D inputs)")
        st = self._fit()
        npar = len(self.params)
        out = np.empty((npar, npar), dtype=DTYPE)
        _lib.check(_lib.load().gpx_gp_dlh_d2lh(st.handle, None, None, _lib.dptr(out)))
        return out

    # ---- prediction (gp/gp.py:504-662) ----
    def Kxoxo(self, xo):
        r""":math:`K(x^*, x^*)`, ``(m, m)``."""
        return self.K(xo, xo)

    def Kxxo(self, xo):
        r""":math:`K(x, x^*)`, ``(n, m)``."""
        return self.K(self._x, xo)

    def Kxox(self, xo):
        r""":math:`K(x^*, x)`, ``(m, n)``."""
        return self.K(xo, self._x)

    def _xo(self, xo):
        return points_arg("xo", xo, self._d)

    def mean(self, xo):
        r"""Predictive mean :math:`K(x^*, x) K_{xx}^{-1} y`, RW06 eq. 2.23 (gp/gp.py:574-597).
        Fused on the device: the ``(m, n)`` cross-kernel matrix is never materialised."""
        st = self._fit_pd()
        xo, m = self._xo(xo)
        out = np.empty(m, dtype=DTYPE)
        lib = _lib.load()
        if native_id(self.K) is not None:
            _lib.check(lib.gpx_gp_mean(st.handle, _lib.dptr(xo), m, _lib.dptr(out)))
        else:
            Kxox = np.ascontiguousarray(self.Kxox(xo), dtype=DTYPE)
            _lib.check(lib.gpx_gp_mean_from_K(st.handle, _lib.dptr(Kxox), m, _lib.dptr(out)))
        return out

    def cov(self, xo):
        r"""Predictive covariance :math:`K(x^*,x^*) - K(x^*,x) K_{xx}^{-1} K(x,x^*)`, RW06
        eq. 2.24 (gp/gp.py:599-625), computed as :math:`K(x^*,x^*) - V^\top V` with
        :math:`V = L^{-1} K(x, x^*)` (no explicit inverse)."""
        st = self._fit_pd()
        xo, m = self._xo(xo)
        out = np.empty((m, m), dtype=DTYPE)
        lib = _lib.load()
        if native_id(self.K) is not None:
            _lib.check(lib.gpx_gp_cov(st.handle, _lib.dptr(xo), m, _lib.dptr(out)))
        else:
            Kxox = np.ascontiguousarray(self.Kxox(xo), dtype=DTYPE)
            Kxoxo = np.ascontiguousarray(self.Kxoxo(xo), dtype=DTYPE)
            _lib.check(lib.gpx_gp_cov_from_K(st.handle, _lib.dptr(Kxox), _lib.dptr(Kxoxo), m,
                                             _lib.dptr(out)))
        return out

    #: plugin kernels: the host evaluates Kxox for `var` in row chunks of at most this many bytes
    _VAR_HOST_CHUNK_BYTES = 256 << 20

    def var(self, xo, noise=False, chunk_rows=0):
        r"""Predictive variance, the diagonal of `cov(xo)` (RW06 eq. 2.24), ``(m,)`` -- at any `m`: the test points go
        through the device in row chunks (:math:`X = K(x^*_c, x) L^{-\top}`, then
        :math:`k(x^*_i, x^*_i) - \sum_j X_{ij}^2`), so nothing ``(m, m)`` and no whole ``(m, n)`` matrix exists on the
        device, on the host or in between.  ``noise=True`` adds :math:`s^2` (the variance of a new observation).
        ``chunk_rows``: rows per device chunk, 0 (automatic) or a multiple of 128.  Like the diagonal of `cov`, the
        result is NOT clamped at zero: where the posterior variance is below the rounding error of the two terms it
        may come out slightly negative."""
        xo, m = self._xo(xo)                         # a bad shape raises before the library is touched
        chunk_rows = chunk_arg("chunk_rows", chunk_rows)
        st = self._fit_pd()
        out = np.empty(m, dtype=DTYPE)
        lib = _lib.load()
        if native_id(self.K) is not None:
            _lib.check(lib.gpx_gp_var(st.handle, _lib.dptr(xo), m, chunk_rows, _lib.dptr(out)))
        else:
            step = max(1, self._VAR_HOST_CHUNK_BYTES // (8 * self._n))
            for r0 in range(0, m, step):
                xc = xo[r0:r0 + step]
                Kxox = np.ascontiguousarray(self.Kxox(xc), dtype=DTYPE)
                kdiag = np.ascontiguousarray(self.K.diag(xc), dtype=DTYPE)
                _lib.check(lib.gpx_gp_var_from_K(st.handle, _lib.dptr(Kxox), _lib.dptr(kdiag), xc.shape[0], chunk_rows,
                                                 _lib.dptr(out[r0:r0 + step])))
        if noise:
            out += self._s ** 2
        return out

    def predict(self, xo, noise=False):
        r"""``(mean(xo), var(xo, noise))``: the predictive mean and its error bar, both ``(m,)``."""
        xo, _ = self._xo(xo)
        return self.mean(xo), self.var(xo, noise=noise)

    # ---- input-space gradients of the prediction (extension) ----
    def _grad_args(self, xo, chunk_rows, name):
        """(xo, m, chunk_rows, the fitted state) of a gradient call; every refusal comes before the library is touched."""
        xo, m = self._xo(xo)
        chunk_rows = chunk_arg("chunk_rows", chunk_rows)
        if native_id(self.K) is None:
            raise NotImplementedError("%s needs a built-in kernel: the kernel plugin contract (K, jacobian, hessian) has no "
                                      "derivative with respect to the inputs, dk/dx" % name)
        return xo, m, chunk_rows, self._fit_pd()

    def dmean_dx(self, xo):
        r"""Gradient of the predictive mean with respect to the test point,
        :math:`\partial m(x^*_i) / \partial x^*_i = \sum_j \alpha_j \, \partial k(x^*_i, x_j) / \partial x^*_i`, float64 in the
        shape of `xo` (``(m,)`` for 1-D inputs, ``(m, d)`` otherwise).  One fused device pass; no ``(m, n)`` matrix exists."""
        xo, m, _, st = self._grad_args(xo, 0, "dmean_dx")
        out = np.empty(xo.shape, dtype=DTYPE)
        _lib.check(_lib.load().gpx_gp_mean_grad(st.handle, _lib.dptr(xo), m, _lib.dptr(out)))
        return out

    def _var_grad(self, xo, chunk_rows, name, want_var):
        xo, m, chunk_rows, st = self._grad_args(xo, chunk_rows, name)
        grad = np.empty(xo.shape, dtype=DTYPE)
        var = np.empty(m, dtype=DTYPE) if want_var else None
        _lib.check(_lib.load().gpx_gp_var_grad(st.handle, _lib.dptr(xo), m, chunk_rows,
                                               _lib.dptr(var) if want_var else None, _lib.dptr(grad)))
        return var, grad

    def dvar_dx(self, xo, chunk_rows=0):
        r"""Gradient of the predictive variance `var(xo)` with respect to the test point,
        :math:`-2 \sum_j \beta_{ij} \, \partial k(x^*_i, x_j) / \partial x^*_i` with
        :math:`\beta_i = K_{xx}^{-1} k(x, x^*_i)`, float64 in the shape of `xo`.  Row chunks as `var`: per chunk
        :math:`X = K(x^*_c, x)`, :math:`X \leftarrow X L^{-\top}`, :math:`X \leftarrow X L^{-1}`, then one fused pass; no
        :math:`K^{-1}` is formed.  The noise term of ``var(xo, noise=True)`` does not depend on `xo`."""
        return self._var_grad(xo, chunk_rows, "dvar_dx", False)[1]

    def predict_grad(self, xo, noise=False, chunk_rows=0):
        r"""``(mean, var, dmean_dx, dvar_dx)`` at `xo`: what an acquisition function and its optimiser need.  The variance
        comes out of the first sweep of the chunk pass that yields its gradient."""
        var, dvar = self._var_grad(xo, chunk_rows, "predict_grad", True)
        if noise:
            var += self._s ** 2
        return self.mean(xo), var, self.dmean_dx(xo), dvar

    # ---- leave-one-out cross-validation (extension; RW06 section 5.4.2) ----
    @memoprop
    def inv_Kxx_diag(self):
        r"""Diagonal of :math:`K_{xx}^{-1}`, ``(n,)``, without the inverse: :math:`(K^{-1})_{ii} = \|L^{-1} e_i\|^2` from
        the resident factor in row chunks (one :math:`n^3/3` sweep, nothing ``(n, n)`` beside the factor, an ``O(n)``
        download).  Raises numpy.linalg.LinAlgError when `Kxx` is not positive definite, as `inv_Kxx` does."""
        st = self._fit_pd()
        out = np.empty(self._n, dtype=DTYPE)
        _lib.check(_lib.load().gpx_gp_inv_diag(st.handle, 0, _lib.dptr(out)))
        return out

    def loo(self, chunk_rows=0):
        r"""Leave-one-out predictions ``(mean, var, log_p)``, each ``(n,)``, in one device call (RW06 eq. 5.10 - 5.12):
        with :math:`\alpha = K^{-1} y` and :math:`k_i = (K^{-1})_{ii}`,
        :math:`\mu_i = y_i - \alpha_i / k_i`, :math:`\sigma_i^2 = 1 / k_i` and
        :math:`\log p_i = \tfrac12 \log k_i - \tfrac12 \alpha_i^2 / k_i - \tfrac12 \log 2\pi`.
        :math:`\sigma_i^2` is the variance of the left-out OBSERVATION, noise included: ``var(x_i, noise=True)`` of the GP
        fitted without point i.  Fills `loo_mean`, `loo_var` and `loo_log_lh`.  ``chunk_rows`` as for `var`."""
        chunk_rows = chunk_arg("chunk_rows", chunk_rows)
        st = self._fit_pd()
        mean, var, log_p = (np.empty(self._n, dtype=DTYPE) for _ in range(3))
        total = ctypes.c_double(0.0)
        _lib.check(_lib.load().gpx_gp_loo(st.handle, chunk_rows, _lib.dptr(mean), _lib.dptr(var), _lib.dptr(log_p),
                                          ctypes.byref(total)))
        self._memoized.update(loo_mean=mean, loo_var=var, loo_log_lh=DTYPE(total.value))
        return mean, var, log_p

    @memoprop
    def loo_mean(self):
        r"""Leave-one-out predictive mean at every training point, ``(n,)`` (see `loo`)."""
        return self.loo()[0]

    @memoprop
    def loo_var(self):
        r"""Leave-one-out predictive variance of every observation, noise included, ``(n,)`` (see `loo`)."""
        return self.loo()[1]

    @memoprop
    def loo_log_lh(self):
        r"""Leave-one-out log pseudo-likelihood :math:`\sum_i \log p(y_i \mid y_{-i})`, RW06 eq. 5.11 (summed on the
        device in a fixed order); ``-inf`` when `Kxx` is not positive definite, as `log_lh`."""
        if self._fit().info != 0:
            return -np.inf
        self.loo()
        return self._memoized["loo_log_lh"]

    @memoprop
    def dloo_dtheta(self):
        r"""Gradient of `loo_log_lh` with respect to `params`, float64 ``(n_params + 1,)``: RW06 eq. 5.13, rearranged.
        With :math:`W = K^{-1}`, :math:`\alpha = W y`, :math:`k_i = W_{ii}`,

        .. math::
            c_i = \tfrac12 (1 + \alpha_i^2 / k_i) / k_i, \quad r = W (\alpha / k), \quad P = W \,\mathrm{diag}(c)\, W, \quad
            G = \tfrac12 (r \alpha^\top + \alpha r^\top) - P,

        .. math::
            \partial L_{LOO} / \partial \theta_j = \sum_{ab} (\partial K / \partial \theta_j)_{ab} G_{ab}, \qquad
            \partial L_{LOO} / \partial s = 2 s \,(r \cdot \alpha - \mathrm{tr}\, P).

        Eq. 5.13 as printed takes one :math:`n^3` product per parameter; this form takes ONE for all of them
        (:math:`P = Y Y^\top`, :math:`Y = W \mathrm{diag}(\sqrt{c})`, lower triangle).  Cost: what `dloglh_dtheta` costs
        (:math:`K^{-1}` from the factor, :math:`n^3`) plus that product (:math:`n^3`) and one fused pass over :math:`P`;
        device memory the factor plus two ``(n, n)`` blocks, the same as `dloglh_dtheta`.  Native kernels (the
        eligibility of `dloglh_dtheta`'s device route): everything on the device, :math:`r` by two triangular solves,
        the kernel derivatives evaluated on the fly; `loo_log_lh` comes out of the same call and is filled when absent.
        Every other kernel (plugin kernels, periodic at d > 1): :math:`G` is downloaded once and contracted with
        `Kxx_J` on the host; it is not kept.  All NaN when `Kxx` is not positive definite, as `dloglh_dtheta`."""
        npar = len(self.params)
        st = self._fit()
        out = np.empty(npar, dtype=DTYPE)
        if st.info != 0:
            out.fill(np.nan)
            return out
        if device_grad(native_id(self.K), self._d):
            total = ctypes.c_double(0.0)
            _lib.check(_lib.load().gpx_gp_loo_grad(st.handle, ctypes.byref(total), _lib.dptr(out)))
            self._memoized.setdefault("loo_log_lh", DTYPE(total.value))
            return out
        G = np.empty((self._n, self._n), dtype=DTYPE)
        _lib.check(_lib.load().gpx_gp_loo_grad_weights(st.handle, _lib.dptr(G), self._n))
        J = self.Kxx_J
        for j in range(npar - 1):
            out[j] = np.sum(J[j] * G)
        out[npar - 1] = 2.0 * self._s * np.trace(G)
        return out

    def dm_dtheta(self, xo):
        r"""Derivative of the predictive mean w.r.t. the parameters, ``(n_p, m)``
        (gp/gp.py:627-662, gp_c.pyx:114-131)."""
        self._no_ard("dm_dtheta")
        if self._native_derivs():
            st = self._fit_pd()                      # LinAlgError when not PD, as inv_Kxx raises in the reference
            xo, m = self._xo(xo)
            dm = np.empty((len(self.params), m), dtype=DTYPE)
            _lib.check(_lib.load().gpx_gp_dm_dtheta(st.handle, _lib.dptr(xo), m, _lib.dptr(dm)))
            return dm
        Ki = self.inv_Kxx
        Kj = _c(self.Kxx_J)
        Kjxo = _c(self.K.jacobian(xo, self._x))
        Kxox = _c(self.Kxox(xo))
        dm = np.empty((len(self.params), Kxox.shape[0]))
        gp_c.dm_dtheta(_c(self._y), Ki, Kj, Kjxo, Kxox, self._s, dm)
        return dm

    # ---- persistence of the DEVICE state (extension; the reference pickles host arrays, gp/gp.py:78-92) ----
    def save_fitted(self, path):
        """Checkpoint the fitted device state -- x, y, alpha and the Cholesky factor -- to `path`,
        streamed from HBM in row blocks (host memory use does not grow with n; a 32 GiB factor never
        needs a host copy).  Restore with `GP.load_fitted`."""
        st = self._fit()
        _lib.check(_lib.load().gpx_gp_save(st.handle, str(path).encode()))

    @classmethod
    def load_fitted(cls, path, K=None, device=None):
        """A GP restored from `save_fitted`: the factor goes straight back into HBM and nothing is
        recomputed (`log_lh`, `mean`, `cov`, ... are served from the loaded state).  `K`: the kernel
        object for a plugin kernel; built-in kernels are rebuilt from the file."""
        lib = select_device(device)
        h = ctypes.c_void_p()
        _lib.check(lib.gpx_gp_load(ctypes.byref(h), str(path).encode()))
        try:
            dt, kid, n, d, info = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int(), ctypes.c_int(0)
            prm = np.zeros(3)
            s = ctypes.c_double()
            _lib.check(lib.gpx_gp_describe(h, ctypes.byref(dt), ctypes.byref(kid), ctypes.byref(n), ctypes.byref(d),
                                           _lib.dptr(prm), ctypes.byref(s)))
            x = np.empty((n.value, d.value), dtype=DTYPE)
            y = np.empty(n.value, dtype=DTYPE)
            _lib.check(lib.gpx_gp_get_xy(h, _lib.dptr(x), _lib.dptr(y)))
            _lib.check(lib.gpx_gp_info(h, ctypes.byref(info)))
            if K is None and kid.value == _lib.KERNEL_GAUSSIAN_ARD:
                full, cnt = np.zeros(1 + _lib.ARD_MAX_D), ctypes.c_int(0)
                _lib.check(lib.gpx_gp_get_params(h, _lib.dptr(full), full.size, ctypes.byref(cnt)))
                K = kernel_class(kid.value)(full[0], full[1:cnt.value])
            elif K is None:
                K = kernel_class(kid.value)(*prm[:FAMILIES[kid.value].nparams(d.value)])
            if d.value == 1 and kid.value != _lib.KERNEL_GAUSSIAN_ARD:
                x = x.ravel()
        except Exception:
            lib.gpx_gp_destroy(h)
            raise
        return cls._adopt_fitted(h, kid.value, info.value, K, x, y, s.value, dt.value, device)

    @classmethod
    def _adopt_fitted(cls, handle, kid, info, K, x, y, s, dtype_id, device):
        """A GP on ``(K, x, y, s)`` whose device state is the fitted gpx_gp `handle` (family `kid`, fit status `info`): nothing
        is uploaded or refitted until an input changes.  The handle is destroyed when the object cannot be built."""
        try:
            obj = cls(K, x, y, s=s, dtype=dtype_name(dtype_id), device=device)
            st = _DeviceState(obj._dtype, kid, obj._n, obj._d, obj._device, handle=handle)
        except Exception:
            _lib.load().gpx_gp_destroy(handle)
            raise
        st.info = info
        st.data_version = obj._data_version
        st.params_version = st.fit_version = obj._version
        obj._dev = st
        return obj

    # ---- joint posterior samples (extension) ----
    def _auto_jitter(self, xo, Kxoxo=None):
        """``sqrt(eps_dtype) * k(0)``: the prior variance from the kernel's closed form, or -- a plugin kernel -- the largest
        diagonal entry of the `Kxoxo` it evaluated."""
        k0 = np.max(self.K.diag(xo[:1])) if Kxoxo is None else np.max(np.diag(Kxoxo))
        return float(np.sqrt(dtype_eps(self._dtype)) * k0)

    def sample(self, xo, size=None, seed=None, noise=False, jitter=None):
        r"""Draws from the joint posterior of the function values at `xo`, on the device:
        :math:`f = m(x^*) + L_c z` with :math:`L_c L_c^\top = \mathrm{cov}(x^*) + \epsilon I` and `z` standard normal --
        the covariance is the matrix `cov(xo)` returns, factored where it was built, and only the samples come back.
        Float64, ``(m,)`` for ``size=None`` and ``(size, m)`` for an int ``size >= 0``; ``sample(xo, seed=k)`` is
        ``sample(xo, size=1, seed=k)[0]``.

        ``seed``: an int in ``[0, 2**64)`` -- the same seed gives the same bits, on any device and for any `size` prefix
        of rows; ``None`` takes one from numpy's global state (``np.random.randint``), so ``np.random.seed`` governs it.
        The normal numbers are the counter-based sequence of ``gpx_d_randn`` (include/gpx.h), stream 0: row `s`, point `i`
        is element ``s * m + i``.  ``noise=True`` adds :math:`s^2` to the diagonal: the draw is of new observations.
        ``jitter``: :math:`\epsilon \ge 0`; ``None`` is ``sqrt(eps_dtype) * k(0)`` with `k(0)` the kernel's prior variance
        (a plugin kernel: the largest diagonal entry of ``Kxoxo(xo)``).  A posterior covariance is singular to rounding
        wherever `xo` comes close to the data or to itself; when the factorisation still fails, numpy.linalg.LinAlgError
        names the pivot and the jitter -- nothing is retried with a larger one.  Memory: ``(m, n)``, ``(m, m)`` and two
        ``(size, m)`` blocks on the device; `m` is bounded by HBM."""
        xo, m = self._xo(xo)                         # every refusal comes before the library is touched
        size = count_arg("size", size, 0, none_ok=True)
        S = 1 if size is None else size
        seed = seed_arg(seed)
        jitter = nonneg_float_arg("jitter", jitter, sample_wording=True)
        st = self._fit_pd()
        lib = _lib.load()
        out = np.empty((S, m), dtype=DTYPE)
        info = ctypes.c_int(0)
        if native_id(self.K) is not None:
            _lib.check(lib.gpx_gp_sample(st.handle, _lib.dptr(xo), m, S, seed, int(bool(noise)), -1.0 if jitter is None else jitter,
                                         _lib.dptr(out), ctypes.byref(info)))
            if info.value != 0 and jitter is None:
                jitter = self._auto_jitter(xo)
        else:
            # (no K() of an empty point set; and the handle of a plugin kernel was fitted from an uploaded matrix: it holds
            # no s, so s^2 rides in the jitter)
            Kxox = np.ascontiguousarray(self.Kxox(xo), dtype=DTYPE) if m else None
            Kxoxo = np.ascontiguousarray(self.Kxoxo(xo), dtype=DTYPE) if m else None
            if jitter is None:
                jitter = self._auto_jitter(xo, Kxoxo) if m else 0.0
            _lib.check(lib.gpx_gp_sample_from_K(st.handle, _lib.dptr(Kxox) if m else None, _lib.dptr(Kxoxo) if m else None, m, S,
                                                seed, 0, jitter + (float(self._s) ** 2 if noise else 0.0), _lib.dptr(out),
                                                ctypes.byref(info)))
        if info.value != 0:
            raise np.linalg.LinAlgError("the posterior covariance at xo plus jitter %.3e is not positive definite: pivot %d of %d "
                                        "is not positive (pass a larger jitter)" % (jitter, info.value, m))
        return out[0] if size is None else out

    # ---- posterior function samples (extension) ----
    def sample_paths(self, size, seed=None, features=1024):
        r"""`size` draws of the posterior FUNCTION as a `PosteriorPaths` object that is evaluated at any number of points
        afterwards, ``paths(xo) -> (size, m)``: pathwise conditioning (Matheron's rule),
        :math:`f_s(a) = \phi(a)^\top \Theta_s + k(a, x) K_{xx}^{-1} (y - \Phi(x) \Theta_s - s\,\epsilon_s)` -- a
        random-feature draw of the prior (`features` frequencies, cos / sin pairs) plus an exact, data-dependent update.
        Where `sample` factors an ``(m, m)`` covariance for one fixed point set, a path costs ``O(m n)`` per evaluation and
        can be optimised over many candidates (Thompson sampling).  `gaussian_processes_amd.paths` has the definition of
        every random input; the object is a pure function of ``(seed, size, features)`` and this fitted GP.

        ``size``: an int ``>= 0``.  ``seed``: as in `sample` (an int in ``[0, 2**64)``; ``None`` draws one from numpy's
        global state); row `s` depends on `s` alone, so ``sample_paths(3, seed)`` is a prefix of ``sample_paths(9, seed)``.
        ``features``: an int ``>= 1``; the prior's covariance error is ``O(k0 / sqrt(features))`` with `k0` the prior
        variance, the data update is exact.  The draws are of the latent function: observation noise is not added.
        Memory held on the device until the object is closed or collected: ``size x n`` weights (plus ``size x 2 features``
        and a copy of `x`).  The result does not refer to this GP again.

        `GaussianKernel` and `GaussianARDKernel` only: NotImplementedError for `PeriodicKernel` and for plugin kernels.
        Raises numpy.linalg.LinAlgError when `Kxx` is not positive definite.

        The paths are differentiable in their input: ``paths.grad(xo) -> (size,) + xo.shape`` and
        ``paths.value_and_grad(xo) -> (values, grad)`` give :math:`\partial f_s / \partial a_k` at every point from one
        fused pass, so a draw can be maximised by a gradient-based multi-start optimiser rather than by central differences.
        Not offered: second derivatives, `DistributedGP`, persistence of paths."""
        from .paths import PosteriorPaths
        size = count_arg("size", size, 0)            # every refusal comes before the library is touched
        features = count_arg("features", features, 1)
        seed = seed_arg(seed)
        if not has_paths(native_id(self.K)):
            raise NotImplementedError("sample_paths supports GaussianKernel and GaussianARDKernel (a random-feature prior needs "
                                      "the kernel's spectral density); %s is not supported" % type(self.K).__name__)
        st = self._fit_pd()
        h = ctypes.c_void_p()
        _lib.check(_lib.load().gpx_gp_paths_create(st.handle, size, features, seed, ctypes.byref(h)))
        return PosteriorPaths(h, size, features, seed, self._n, self._d, self._x.ndim)

    # ---- growing a fitted GP (extension) ----
    def extend(self, x_new, y_new):
        r"""A new, fitted `GP` on the data of this one plus `k` further observations, without refactoring: the Cholesky
        factor of the bordered matrix is the old factor with `k` rows appended,
        :math:`X = K(x_{new}, x) L^{-\top}` and the factor of :math:`K(x_{new}, x_{new}) + s^2 I - X X^\top`.  One
        triangular sweep over `k` right-hand sides (:math:`O(n^2 k)`) and two solves for the new :math:`K^{-1} y`
        (:math:`O(n^2)`), against :math:`n^3/3` for ``g.x = ...; g.y = ...``.  ``x_new``: ``(k,)`` for 1-D inputs or
        ``(k, d)``; ``y_new``: ``(k,)``; ``k >= 1``.  The result carries a deep copy of `K` and the same `s`, `dtype` and
        `device`; this object and its device state are unchanged.  Raises numpy.linalg.LinAlgError when this GP's
        `Kxx` is not positive definite; when the extended matrix is not, the result behaves like any GP whose fit
        failed (``log_lh == -inf``, `Lxx` raises).

        Memory: source and result coexist, so TWO factors are resident in HBM (:math:`n^2 + (n + k)^2` elements)
        until the source is dropped; ``g = g.extend(xn, yn)`` releases it."""
        x_new = np.ascontiguousarray(x_new, dtype=DTYPE)       # every refusal comes before the library is touched
        y_new = np.ascontiguousarray(y_new, dtype=DTYPE)
        if x_new.ndim != self._x.ndim or (x_new.ndim == 2 and x_new.shape[1] != self._d):
            raise ValueError("invalid shape for x_new: %s" % str(x_new.shape))
        k = x_new.shape[0]
        if k < 1:
            raise ValueError("extend needs at least one new point (k = %d)" % k)
        if y_new.shape != (k,):
            raise ValueError("invalid shape for y_new: %s" % str(y_new.shape))
        K, x, y = deepcopy(self.K), np.concatenate([self._x, x_new]), np.concatenate([self._y, y_new])
        st = self._fit_pd()
        lib = _lib.load()
        h, info = ctypes.c_void_p(), ctypes.c_int(0)
        if native_id(self.K) is not None:
            _lib.check(lib.gpx_gp_extend(st.handle, _lib.dptr(x_new), _lib.dptr(y_new), k, ctypes.byref(h), ctypes.byref(info)))
        else:
            Kno = np.ascontiguousarray(self.K(x_new, self._x), dtype=DTYPE)
            Knn = np.array(self.K(x_new, x_new), dtype=DTYPE, order="C")
            Knn[np.diag_indices_from(Knn)] += self._s ** 2
            check_finite(Kno)
            check_finite(Knn)
            _lib.check(lib.gpx_gp_extend_from_K(st.handle, _lib.dptr(x_new), _lib.dptr(y_new), k, _lib.dptr(Kno),
                                                _lib.dptr(Knn), ctypes.byref(h), ctypes.byref(info)))
        return self._adopt_fitted(h, st.key[1], info.value, K, x, y, self._s, self._dtype, self._device)

    # ---- shrinking a fitted GP ----
    def _removal_indices(self, idx):
        """`idx` of `remove` as a sorted int64 array of distinct indices in [0, n), fewer than n of them; ValueError otherwise."""
        n = self._n
        a = np.asarray(idx)
        if a.dtype == np.bool_:
            if a.shape != (n,):
                raise ValueError("invalid shape for a boolean mask: %s, expected (%d,)" % (str(a.shape), n))
            a = np.flatnonzero(a)
        else:
            if a.ndim == 0:
                a = a.reshape(1)
            if a.ndim != 1:
                raise ValueError("idx must be an int, a 1-D sequence of ints or a boolean mask of shape (n,)")
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError("idx must hold integers, not %s" % a.dtype)
        if a.size == 0:
            raise ValueError("remove needs at least one index")
        a = a.astype(np.int64)
        if ((a < -n) | (a >= n)).any():
            raise ValueError("index out of range for %d points" % n)
        a = np.sort(np.where(a < 0, a + n, a))
        if (a[1:] == a[:-1]).any():
            raise ValueError("idx holds an index more than once")
        if a.size >= n:
            raise ValueError("cannot remove all %d points" % n)
        return np.ascontiguousarray(a)

    def remove(self, idx):
        r"""A new, fitted `GP` on the data of this one without the observations `idx`, without refactoring.  Deleting
        row and column `i` of :math:`K = L L^\top` leaves the factor before `i` as it is; the part behind it takes the
        rank-1 update :math:`L_{33}' L_{33}'^\top = L_{33} L_{33}^\top + l_{32} l_{32}^\top` by Givens rotations --
        unconditionally stable, and no kernel is evaluated, so every family and every plugin kernel takes the same path.
        Cost: :math:`O((n - r_0)^2 k)` for `k` indices of which :math:`r_0` is the smallest -- all `k` updates share ONE
        pass, so the trailing triangle moves once -- and two solves for the new :math:`K^{-1} y` (:math:`O(n^2)`),
        against :math:`n^3/3` for ``g.x = ...; g.y = ...``.

        `idx`: an int, a 1-D sequence of ints (negative values count from the end; any order) or a boolean mask of
        shape ``(n,)``.  ValueError for an empty `idx`, an index twice, an index out of range, all `n` points, or a
        non-integer dtype.  The result has ``np.delete(x, idx, axis=0)`` and ``np.delete(y, idx)``, a deep copy of `K`
        and the same `s`, `dtype` and `device`; this object and its device state are unchanged.  Raises
        numpy.linalg.LinAlgError when this GP's `Kxx` is not positive definite.

        Memory: source and result coexist, so TWO factors are resident in HBM (:math:`n^2 + (n - k)^2` elements) until
        the source is dropped; ``g = g.remove(i)`` releases it.  A sliding window is
        ``g = g.extend(xn, yn).remove(range(k))``."""
        rm = self._removal_indices(idx)                        # every refusal comes before the library is touched
        K, x, y = deepcopy(self.K), np.delete(self._x, rm, axis=0), np.delete(self._y, rm)
        st = self._fit_pd()
        h, info = ctypes.c_void_p(), ctypes.c_int(0)
        _lib.check(_lib.load().gpx_gp_remove(st.handle, rm.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), int(rm.size), ctypes.byref(h),
                                             ctypes.byref(info)))
        return self._adopt_fitted(h, st.key[1], info.value, K, x, y, self._s, self._dtype, self._device)

    def fit_timing(self):
        """Milliseconds of the last device fit: kernel build, potrf, solve, reductions, total
        (HIP events on the handle's stream)."""
        return timing("gpx_gp_last_timing", self._fit().handle, ("kernel_build", "potrf", "solve", "reduce", "total"))

    def plot(self, ax=None, xlim=None, color="k", markercolor="r"):
        """Plot the predictive mean +/- one standard deviation (gp/gp.py:664-700)."""
        import matplotlib.pyplot as plt
        x, y = self._x, self._y
        if ax is None:
            ax = plt.gca()
        if xlim is None:
            xlim = (x.min(), x.max())
        X = np.linspace(xlim[0], xlim[1], 1000)
        mean = self.mean(X)
        std = np.sqrt(np.diag(self.cov(X)))
        ax.fill_between(X, mean - std, mean + std, color=color, alpha=0.3)
        ax.plot(X, mean, lw=2, color=color)
        ax.plot(x, y, "o", ms=5, color=markercolor)
        ax.set_xlim(*xlim)


def _c(a):
    """float64 C-contiguous view / copy (what the ext modules' buffer arguments require)."""
    return np.ascontiguousarray(a, dtype=DTYPE)
