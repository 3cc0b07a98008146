"""SparseGP -- GP regression on M inducing points (Titsias 2009, the collapsed bound; "SGPR") on MI355X.

The dense `GP` factors an n x n matrix; this class never forms one.  With inducing inputs `z` (M, d)::

    Kuu  = K(z, z) + jitter I = Luu Luu^T       Phi = K(z, x) K(x, z)        b = K(z, x) y
    X    = Luu^-1 Phi Luu^-T                    B = I + X / s^2 = LB LB^T    c = LB^-1 Luu^-1 b / s
    elbo = -sum log diag LB - N/2 log 2 pi - N log s - y.y / (2 s^2) + c.c / (2 s^2) - (sum_i k(x_i, x_i) - tr X) / (2 s^2)
    mean(a) = k(a, z) Luu^-T LB^-T c / s
    var(a)  = k(a, a) - |Luu^-1 k(z, a)|^2 + |LB^-1 Luu^-1 k(z, a)|^2

O(N M^2) time, O(M^2 + M chunk) device memory: x passes through the device in column chunks (``gpx_sgp_fit``,
include/gpx.h).  `elbo` is a LOWER BOUND on the log marginal likelihood of the dense GP, not that likelihood: there is no
attribute called ``log_lh`` here, on purpose.

`delbo_dtheta` is the gradient of the bound in ``(kernel parameters..., s)`` with `z` and the jitter held fixed
(``gpx_sgp_grad``: a second pass over the chunks of `x`), `delbo_dz` the gradient in the inducing inputs from the same pass
(``gpx_sgp_grad_z``), `optimize` an L-BFGS-B on top of either: over the parameters, or with ``inducing=True`` over the
parameters and `z` together.  `SparseGP.greedy_inducing` chooses the `z` to start from: greedy conditional-variance selection
among the rows of `x` (``gpx_sgp_select``), which depends on the kernel and `x` alone.
"""
import ctypes

import numpy as np

from . import _lib
from ._facade import (DTYPE, Handle, ParamsMixin, check_finite, chunk_arg, dtype_eps, dtype_id, native_id, nonneg_float_arg,
                      points_arg, select_device, timing)

__all__ = ["SparseGP"]

ELBO_TERMS = ("logdet", "noise", "fit", "quad", "trace")
_STAGE_NAMES = {1: "Kuu = K(z, z) + jitter I", 2: "B = I + Luu^-1 Phi Luu^-T / s^2"}


class _SparseState(Handle):
    """Owns the gpx_sgp handle of one SparseGP; rebuilt whenever a shape, the dtype or the kernel family changes."""
    _destroy = "gpx_sgp_destroy"

    def __init__(self, dtype_id, kernel_id, n, m, d, device):
        Handle.__init__(self)
        self.key = (dtype_id, kernel_id, n, m, d, device)
        self.xy_version = self.z_version = self.fit_version = -1
        self.stage = self.pivot = None
        _lib.check(select_device(device).gpx_sgp_create(ctypes.byref(self.handle), dtype_id, kernel_id, n, m, d))


def _changed(val, cur):
    """Does `val` differ from the array `cur` (None: nothing there yet) in shape or in any element?"""
    if cur is None:
        return True
    val = np.asarray(val)
    return val.shape != cur.shape or bool(np.any(val != cur))


def _native_id(K, d=None):
    """The library's id of a built-in kernel (a plugin kernel has none); with `d`, an ARD kernel must have that many widths."""
    kid = native_id(K, d)
    if kid is None:
        raise NotImplementedError("SparseGP needs a built-in kernel (GaussianKernel, PeriodicKernel, GaussianARDKernel): "
                                  "plugin kernels are not supported")
    return kid


def _points(name, val, K=None, copy=False):
    """``(array, d)``: `val` as finite float64 points ``(n,)`` or ``(n, d)``, ``n >= 1`` (`copy`: never a view of `val`); with
    `K`, checked against it (`_native_id`)."""
    arr = np.array(val, copy=True, dtype=DTYPE) if copy else np.ascontiguousarray(val, dtype=DTYPE)
    if arr.ndim not in (1, 2) or arr.shape[0] < 1:
        raise ValueError("invalid shape for %s: %s" % (name, str(arr.shape)))
    check_finite(arr)
    d = 1 if arr.ndim == 1 else arr.shape[1]
    if K is not None:
        _native_id(K, d)
    return arr, d


def _k0_jitter(K, point, dtype_id):
    """``sqrt(eps_dtype) * k(0)`` at `point` (one row): the automatic jitter, and `greedy_inducing`'s automatic `tol`."""
    return float(np.sqrt(dtype_eps(dtype_id)) * np.max(K.diag(point)))


class SparseGP(ParamsMixin):
    r"""Sparse GP regression on inducing points.

    Parameters
    ----------
    K : one of the built-in kernels (`GaussianKernel`, `PeriodicKernel`, `GaussianARDKernel`)
    x : ``(n,)`` or ``(n, d)`` input locations;  y : ``(n,)`` observations
    s : standard deviation of the observation noise, ``> 0`` (the bound divides by :math:`s^2`)
    z : ``(M,)`` or ``(M, d)`` inducing inputs, ``M >= 1`` (`greedy_inducing` selects rows of `x`, `subset_inducing` draws them)
    jitter : added to the diagonal of ``K(z, z)``; ``None`` is ``sqrt(eps_dtype) * k(0)``
    chunk_cols : columns of `x` per device chunk of the fit, 0 (automatic) or a multiple of 128
    """

    def __init__(self, K, x, y, s, z, jitter=None, dtype="float64", device=None, chunk_cols=0):
        _native_id(K)
        self.K = K
        self._x = self._y = self._z = self._s = None
        self._dtype = dtype_id(dtype)
        self._device = device
        self._dev = None
        self._version = 0          # bumped by every invalidation
        self._data_version = 0     # bumped when x, y or z change
        self._xy_version = 0       # ... when x or y change: everything is uploaded again
        self._z_version = 0        # ... when z changes: only z is uploaded
        self._memoized = {}
        self._jitter = None
        self._chunk_cols = 0
        self.x = x
        self.y = y
        self.z = z
        self.s = s
        self.jitter = jitter
        self.chunk_cols = chunk_cols

    # ---- invalidation: GP's scheme ----
    def _invalidate(self, data=False, z=False):
        self._memoized = {}
        self._version += 1
        if data or z:
            self._data_version += 1
        if data:
            self._xy_version += 1
        if z:
            self._z_version += 1

    @property
    def x(self):
        return self._x

    @x.setter
    def x(self, val):
        if _changed(val, self._x):
            arr = _points("x", val, copy=True)[0]    # (an ARD kernel's widths: `_state`, with the kernel as it is then)
            self._invalidate(data=True)
            self._x = arr
            self._x.flags.writeable = False

    @property
    def y(self):
        return self._y

    @y.setter
    def y(self, val):
        if _changed(val, self._y):
            arr = np.array(val, copy=True, dtype=DTYPE)
            if arr.shape != (self._x.shape[0],):
                raise ValueError("invalid shape for y: %s" % str(arr.shape))
            check_finite(arr)
            self._invalidate(data=True)
            self._y = arr
            self._y.flags.writeable = False

    @property
    def z(self):
        r"""Inducing inputs, read-only float64 copy, in the shape they were given."""
        return self._z

    @z.setter
    def z(self, val):
        if _changed(val, self._z):
            arr = np.array(val, copy=True, dtype=DTYPE)
            d = 1 if arr.ndim == 1 else (arr.shape[1] if arr.ndim == 2 else -1)
            if arr.ndim not in (1, 2) or d != self._d:
                raise ValueError("invalid shape for z: %s (x has %d dimension(s))" % (str(arr.shape), self._d))
            if arr.shape[0] < 1:
                raise ValueError("need at least one inducing point (M >= 1)")
            check_finite(arr)
            self._invalidate(z=True)
            self._z = arr
            self._z.flags.writeable = False

    @property
    def s(self):
        return self._s

    @s.setter
    def s(self, val):
        if not (val > 0) or not np.isfinite(val):
            raise ValueError("invalid value for s: %s (the bound divides by s^2: s > 0)" % val)
        if val != self._s:
            self._invalidate()
            self._s = DTYPE(val)

    @property
    def jitter(self):
        r"""The value in force: the one given, or ``sqrt(eps_dtype) * k(0)`` from the kernel's current parameters."""
        return _k0_jitter(self.K, self._z[:1], self._dtype) if self._jitter is None else self._jitter

    @jitter.setter
    def jitter(self, val):
        val = nonneg_float_arg("jitter", val)
        if val != self._jitter:
            self._invalidate()
            self._jitter = val

    @property
    def chunk_cols(self):
        return self._chunk_cols

    @chunk_cols.setter
    def chunk_cols(self, val):
        val = chunk_arg("chunk_cols", val)
        if val != self._chunk_cols:
            self._invalidate()
            self._chunk_cols = val

    @property
    def n_inducing(self):
        return self._z.shape[0]

    @property
    def _n(self):
        return self._x.shape[0]

    @property
    def _d(self):
        return 1 if self._x.ndim == 1 else self._x.shape[1]

    @staticmethod
    def subset_inducing(x, M, seed=0):
        r"""`M` distinct rows of `x`, in the order ``numpy.random.RandomState(seed).permutation(n)[:M]`` gives: a pure
        function of ``(x.shape, M, seed)`` where the choice of rows is concerned."""
        x = np.asarray(x)
        M = int(M)
        if x.ndim not in (1, 2):
            raise ValueError("invalid shape for x: %s" % str(x.shape))
        if M < 1 or M > x.shape[0]:
            raise ValueError("invalid value for M: %d (1 .. %d)" % (M, x.shape[0]))
        return np.array(x[np.random.RandomState(seed).permutation(x.shape[0])[:M]], dtype=DTYPE)

    @staticmethod
    def greedy_inducing(K, x, M, tol=None, first=None, dtype="float64", device=None, return_info=False, factor=False):
        r"""Up to `M` rows of `x` chosen by greedy conditional-variance selection (Burt, Rasmussen and van der Wilk 2020; a
        pivoted partial Cholesky of ``K(x, x)``, on the device: ``gpx_sgp_select``).  Every step takes the point whose prior
        variance GIVEN the points already taken is largest (on a tie the smallest index; step 0 takes row `first` when it
        is given).  The choice depends on the kernel and `x` alone -- not on `y` or `s` -- and is deterministic.

        Returns ``x[index]`` as float64, ``(count, d)`` or ``(count,)`` for 1-D `x`: exact copies of rows of `x`, in the
        order picked.  The selection stops early once no remaining point has a conditional variance above `tol`, so
        ``count < M`` is NOT an error: the rest of `x` cannot be told apart from the set already picked.  ``tol=None`` is
        ``sqrt(eps_dtype) * k(0)``, the automatic jitter of the constructor: below it a point is indistinguishable from
        the set once the jitter is on ``K(z, z)``.

        ``return_info=True``: ``(z, info)`` with ``index`` (int64), ``pivot`` (the conditional variance of each pick when
        it was taken), ``trace`` (``count + 1`` values: ``trace[m]`` is :math:`\sum_i k(x_i, x_i) - \mathrm{tr} X` of the
        bound at the first ``m`` picks and jitter 0 -- read it to choose `M`), ``count`` and ``tol``; ``factor=True`` adds
        ``R`` ``(count, n)``, the partial Cholesky factor: ``R.T @ R`` reproduces the picked columns of ``K(x, x)``."""
        kid = _native_id(K)
        xs, d = _points("x", x, K)
        n, M = xs.shape[0], int(M)
        if M < 1 or M > n:
            raise ValueError("invalid value for M: %d (1 .. %d)" % (M, n))
        dt = dtype_id(dtype)
        tol = nonneg_float_arg("tol", tol)
        if first is not None:
            if int(first) != first or not 0 <= int(first) < n:
                raise ValueError("invalid value for first: %s (None, or a row index 0 .. %d)" % (first, n - 1))
            first = int(first)
        if tol is None:
            tol = _k0_jitter(K, xs[:1], dt)
        lib = select_device(device)
        p = np.ascontiguousarray(K.params, dtype=DTYPE)
        index, pivot, trace = np.empty(M, dtype=np.int64), np.empty(M, dtype=DTYPE), np.empty(M + 1, dtype=DTYPE)
        R = np.empty((M, n), dtype=DTYPE) if factor else None
        count = ctypes.c_int64(0)
        _lib.check(lib.gpx_sgp_select(dt, kid, _lib.dptr(xs), n, d, _lib.dptr(p), M, tol, -1 if first is None else first,
                                      index.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _lib.dptr(pivot), _lib.dptr(trace),
                                      None if R is None else _lib.dptr(R), ctypes.byref(count)))
        c = int(count.value)
        index = index[:c].copy()
        z = np.array(xs[index], dtype=DTYPE)
        if not return_info:
            return z
        info = {"index": index, "pivot": pivot[:c].copy(), "trace": trace[:c + 1].copy(), "count": c, "tol": tol}
        if factor:
            info["R"] = R[:c].copy()
        return z, info

    # ---- device plumbing ----
    def _state(self):
        key = (self._dtype, _native_id(self.K, self._d), self._n, self.n_inducing, self._d, self._device)
        if self._dev is None or self._dev.key != key:
            if self._dev is not None:
                self._dev.close()
            self._dev = _SparseState(*key)
        st = self._dev
        if st.xy_version != self._xy_version:
            xs, ys, zs = (np.ascontiguousarray(a, dtype=DTYPE) for a in (self._x, self._y, self._z))
            _lib.check(_lib.load().gpx_sgp_set_data(st.handle, _lib.dptr(xs), _lib.dptr(ys), _lib.dptr(zs)))
            st.xy_version, st.z_version = self._xy_version, self._z_version
            st.fit_version = -1
        elif st.z_version != self._z_version:
            # only z moved (every step of a joint optimisation): x and y stay where they are on the device
            zs = np.ascontiguousarray(self._z, dtype=DTYPE)
            _lib.check(_lib.load().gpx_sgp_set_data(st.handle, None, None, _lib.dptr(zs)))
            st.z_version = self._z_version
            st.fit_version = -1
        return st

    def _fit(self):
        """Make the device state current: one device fit serves `elbo` and every prediction."""
        st = self._state()
        if st.fit_version == self._version:
            return st
        p = np.ascontiguousarray(self.K.params, dtype=DTYPE)
        stage, pivot = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.load().gpx_sgp_fit(st.handle, _lib.dptr(p), float(self._s), float(self.jitter), self._chunk_cols,
                                           ctypes.byref(stage), ctypes.byref(pivot)))
        st.stage, st.pivot = stage.value, pivot.value
        st.fit_version = self._version
        return st

    def _fit_pd(self):
        st = self._fit()
        if st.stage != 0:
            raise np.linalg.LinAlgError("stage %d of the sparse fit (%s): %d-th leading minor of the array is not positive definite"
                                        % (st.stage, _STAGE_NAMES[st.stage], st.pivot))
        return st

    def _elbo_and_terms(self):
        if "elbo" not in self._memoized:
            st = self._fit()
            if st.stage != 0:
                self._memoized["elbo"] = (DTYPE(-np.inf), dict((k, DTYPE(np.nan)) for k in ELBO_TERMS))
            else:
                out, terms = ctypes.c_double(0.0), np.empty(5, dtype=DTYPE)
                _lib.check(_lib.load().gpx_sgp_elbo(st.handle, ctypes.byref(out), _lib.dptr(terms)))
                self._memoized["elbo"] = (DTYPE(out.value), dict(zip(ELBO_TERMS, terms)))
        return self._memoized["elbo"]

    @property
    def elbo(self):
        r"""Titsias' lower bound on the log marginal likelihood, float64; ``-inf`` when either factorisation fails."""
        return self._elbo_and_terms()[0]

    @property
    def elbo_terms(self):
        r"""The five terms of `elbo` (they sum to it): ``logdet`` :math:`-\sum \log \mathrm{diag} L_B`, ``noise``
        :math:`-\frac N2 \log 2\pi - N \log s`, ``fit`` :math:`-y^\top y / 2s^2`, ``quad`` :math:`c^\top c / 2s^2`,
        ``trace`` :math:`-(\sum_i k(x_i, x_i) - \mathrm{tr} X) / 2s^2`."""
        return dict(self._elbo_and_terms()[1])

    # ---- the gradient of the bound and the optimiser on top of it ----
    def _grad(self):
        if "grad" not in self._memoized:
            st = self._fit_pd()
            out = np.empty(self.K.params.size + 1, dtype=DTYPE)
            _lib.check(_lib.load().gpx_sgp_grad(st.handle, self._chunk_cols, _lib.dptr(out)))
            self._memoized["grad"] = out
        return self._memoized["grad"]

    def _grad_z(self):
        """One joint device call: the gradient in z, and the one in the parameters beside it (the bits `_grad` would give)."""
        if "grad_z" not in self._memoized:
            st = self._fit_pd()
            out = np.empty(self.K.params.size + 1, dtype=DTYPE)
            out_z = np.empty((self.n_inducing, self._d), dtype=DTYPE)
            _lib.check(_lib.load().gpx_sgp_grad_z(st.handle, self._chunk_cols, _lib.dptr(out), _lib.dptr(out_z)))
            self._memoized["grad"] = out
            self._memoized["grad_z"] = out_z.reshape(self._z.shape)
        return self._memoized["grad_z"]

    @property
    def delbo_dtheta(self):
        r"""Gradient of `elbo` in `params`, float64 ``(len(params),)`` in their order ``(kernel parameters..., s)``, with
        the inducing inputs held fixed: one ``gpx_sgp_grad`` on the fitted handle (include/gpx.h has the closed form), a
        second pass over `x` in the fit's column chunks.  The JITTER is held at the value in force: it is not
        differentiated, even when ``jitter=None`` makes it follow the kernel's height.  Raises ``LinAlgError`` when a
        factorisation of the fit failed."""
        return self._grad().copy()

    @property
    def delbo_dz(self):
        r"""Gradient of `elbo` in the inducing inputs, float64 in the shape of `z` (``(M, d)`` or ``(M,)``), the parameters and
        the jitter held fixed: one ``gpx_sgp_grad_z`` on the fitted handle, the pass over `x` that `delbo_dtheta` makes with
        one more kernel per chunk -- it leaves `delbo_dtheta` behind too, in the same bits.  Raises ``LinAlgError`` when a
        factorisation of the fit failed."""
        return self._grad_z().copy()

    def elbo_and_grad(self, inducing=False):
        r"""``(elbo, delbo_dtheta)``, the bits of the two properties; ``(-inf, array of NaN)`` when a factorisation failed
        (it does not raise: this is what `optimize` calls at every trial point).  ``inducing=True``: ``(elbo, delbo_dtheta,
        delbo_dz)`` from one joint device call, NaN arrays of both shapes after a failed fit."""
        if self._fit().stage != 0:
            nan = np.full(self.K.params.size + 1, np.nan, dtype=DTYPE)
            return (self.elbo, nan, np.full(self._z.shape, np.nan, dtype=DTYPE)) if inducing else (self.elbo, nan)
        if inducing:
            dz = self.delbo_dz                       # (first: the joint call serves delbo_dtheta)
            return self.elbo, self.delbo_dtheta, dz
        return self.elbo, self.delbo_dtheta

    def grad_timing(self):
        """Milliseconds of the last gradient pass (HIP events on the handle's stream): the M x M part, the chunks' kernel
        builds, their products K(x_c, z) T, their tile reductions, total."""
        self._grad()
        return timing("gpx_sgp_last_grad_timing", self._fit_pd().handle, ("mm", "build", "product", "reduce", "total"))

    def zgrad_timing(self):
        """Milliseconds of the z-gradient's own kernels in the last joint pass: Kuu's share (the pass on `z` against itself),
        the chunks' passes."""
        self._grad_z()
        return timing("gpx_sgp_last_zgrad_timing", self._fit_pd().handle, ("kuu", "chunks"))

    def optimize(self, maxiter=100, bounds=None, inducing=False):
        r"""Maximise `elbo` over `params` (all positive) with scipy's L-BFGS-B in log-parameters, the inducing inputs held
        fixed; one `elbo_and_grad` call per evaluation.  A trial point whose fit fails counts as a very poor one and the
        line search backs off.  `bounds`: ``None``, or one ``(lo, hi)`` pair per parameter in the natural scale (``None``
        for an open end).  The object is left at the best parameters evaluated.  Returns a dict: ``params``, ``elbo``,
        ``nit``, ``nfev``, ``success``, ``message``.

        ``inducing=True``: the inducing inputs move too -- L-BFGS-B over ``(log params, z.ravel())``, one joint device call
        (`elbo_and_grad(inducing=True)`) per evaluation and only `z` uploaded between them.  `z` is unbounded (`bounds` is
        still one pair per parameter), the object is left at the best ``(params, z)`` evaluated and the dict gains ``z``."""
        from scipy.optimize import minimize

        npar, zshape = self.params.size, self._z.shape
        x0 = np.concatenate([np.log(self.params), self._z.ravel()]) if inducing else np.log(self.params)
        if bounds is not None:
            bounds = list(bounds)
            if len(bounds) != npar:
                raise ValueError("bounds: one (lo, hi) pair per parameter (%d), got %d" % (npar, len(bounds)))
            bounds = [tuple(None if b is None else float(np.log(b)) for b in pair) for pair in bounds] + [(None, None)] * (x0.size - npar)
        best = {"elbo": -np.inf, "params": self.params, "z": self._z}
        state = {"worst": None}

        def negative(u):
            self.params = np.exp(u[:npar])
            if inducing:
                self.z = u[npar:].reshape(zshape)
            val, *grads = self.elbo_and_grad(inducing=True) if inducing else self.elbo_and_grad()
            if not (np.isfinite(val) and all(np.all(np.isfinite(g)) for g in grads)):
                # a failed fit: worse than anything seen, flat -- the line search shortens its step
                ref = state["worst"] if state["worst"] is not None else 0.0
                return abs(ref) * 10.0 + 1e10, np.zeros_like(u)
            if val > best["elbo"]:
                best["elbo"], best["params"], best["z"] = float(val), self.params, self._z
            state["worst"] = -val if state["worst"] is None else max(state["worst"], -val)
            grads[0] = np.asarray(grads[0], dtype=DTYPE) * np.exp(u[:npar])             # d/d log theta = theta d/d theta
            return -float(val), -np.concatenate([np.ravel(g) for g in grads])

        res = minimize(negative, x0, jac=True, method="L-BFGS-B", bounds=bounds, options={"maxiter": int(maxiter)})
        self.params = best["params"]                 # (a refit there gives the bits of best["elbo"]: fits are repeatable)
        if inducing:
            self.z = best["z"]
        found = bool(np.isfinite(best["elbo"]))
        msg = res.message.decode() if isinstance(res.message, bytes) else str(res.message)
        out = dict(params=self.params, elbo=DTYPE(best["elbo"]), nit=int(res.nit), nfev=int(res.nfev), success=found and bool(res.success),
                   message=msg if found else "no trial point had a positive definite fit")
        if inducing:
            out["z"] = self._z
        return out

    def _get(self, which):
        if which not in self._memoized:
            st = self._fit_pd()
            M = self.n_inducing
            out = np.empty(M if which in ("c", "b") else (M, M), dtype=DTYPE)
            args = [_lib.dptr(out) if k == which else None for k in ("Luu", "LB", "c", "Phi", "b")]
            _lib.check(_lib.load().gpx_sgp_get(st.handle, *args))
            self._memoized[which] = out
        return self._memoized[which]

    @property
    def Luu(self):
        r"""Lower Cholesky factor of ``K(z, z) + jitter I``, ``(M, M)``."""
        return self._get("Luu")

    @property
    def LB(self):
        r"""Lower Cholesky factor of :math:`B = I + L_{uu}^{-1} \Phi L_{uu}^{-\top} / s^2`, ``(M, M)``."""
        return self._get("LB")

    @property
    def c(self):
        r""":math:`L_B^{-1} L_{uu}^{-1} K(z, x) y / s`, ``(M,)``."""
        return self._get("c")

    @property
    def Phi(self):
        r"""Lower triangle of :math:`K(z, x) K(x, z)`, ``(M, M)``, zero above the diagonal."""
        return self._get("Phi")

    @property
    def b(self):
        r""":math:`K(z, x) y`, ``(M,)``."""
        return self._get("b")

    # ---- predictions ----
    def _xo(self, xo):
        return points_arg("xo", xo, self._d)

    def mean(self, xo):
        r"""Predictive mean :math:`k(x^*, z) L_{uu}^{-\top} L_B^{-\top} c / s`, ``(m,)``: one fused device pass."""
        xo, m = self._xo(xo)
        st = self._fit_pd()
        out = np.empty(m, dtype=DTYPE)
        _lib.check(_lib.load().gpx_sgp_mean(st.handle, _lib.dptr(xo), m, _lib.dptr(out)))
        return out

    def var(self, xo, noise=False, chunk_rows=0):
        r"""Predictive variance, the diagonal of `cov(xo)`, ``(m,)``, in row chunks of `xo` (``chunk_rows``: 0 or a
        multiple of 128).  ``noise=True`` adds :math:`s^2`.  Not clamped at zero."""
        xo, m = self._xo(xo)
        chunk_rows = chunk_arg("chunk_rows", chunk_rows)
        st = self._fit_pd()
        out = np.empty(m, dtype=DTYPE)
        _lib.check(_lib.load().gpx_sgp_var(st.handle, _lib.dptr(xo), m, chunk_rows, _lib.dptr(out)))
        if noise:
            out += self._s ** 2
        return out

    def predict(self, xo, noise=False):
        r"""``(mean(xo), var(xo, noise))``."""
        xo, _ = self._xo(xo)
        return self.mean(xo), self.var(xo, noise=noise)

    def cov(self, xo):
        r"""Predictive covariance :math:`K(x^*, x^*) - V_1^\top V_1 + V_2^\top V_2`, ``(m, m)``."""
        xo, m = self._xo(xo)
        st = self._fit_pd()
        out = np.empty((m, m), dtype=DTYPE)
        _lib.check(_lib.load().gpx_sgp_cov(st.handle, _lib.dptr(xo), m, _lib.dptr(out)))
        return out

    def fit_timing(self):
        """Milliseconds of the last device fit (HIP events on the handle's stream): Kuu and its factor, the chunks' kernel
        builds, the chunks' Gram products (with b and the slice sum), the M x M tail, total."""
        return timing("gpx_sgp_last_timing", self._fit().handle, ("kuu", "build", "gram", "tail", "total"))
