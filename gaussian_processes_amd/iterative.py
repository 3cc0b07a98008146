"""IterativeGP -- exact GP regression past the n x n factor: preconditioned conjugate gradients on MI355X.

`GP` keeps an n x n factor in HBM; `SparseGP` avoids it by approximating.  This class solves the EXACT system::

    (K(x, x) + s^2 I) alpha = y

by conjugate gradients (Gardner et al. 2018; Wang et al. 2019, "Exact GPs on a million data points") and never forms K: a
product with K is one fused pass over the points (``gpx_d_kmat_apply``), and the preconditioner is ``P = R^T R + s^2 I`` with
``R`` the pivoted partial Cholesky of ``K(x, x)`` that `SparseGP.greedy_inducing` computes, applied by Woodbury.  Device memory
is ``8 n (d + 2 rank + 6 S + 2)`` bytes and small change for ``S <= 32`` simultaneous right-hand sides -- nothing scales
with ``n^2`` (``gpx_cg_*``, include/gpx.h; DESIGN 3.3 "Exact GP past the factor").

Model selection stays on the same route: `log_lh_estimate` and `log_lh_and_grad` estimate the marginal likelihood and its
gradient from the CG coefficients of a few random probes (stochastic Lanczos quadrature), the gradient's n^2 contraction runs
in one fused tile reduction whose low-rank coefficients are formed inside the tile (``gpx_d_lowrank_reduce``), and `optimize`
is L-BFGS-B on them with common random numbers.
"""
import ctypes
import warnings

import numpy as np

from . import _lib
from ._facade import (DTYPE, Handle, ParamsMixin, check_finite, count_arg, dtype_eps, dtype_id, native_id, points_arg,
                      select_device, timing)
from .sparse import _changed, _k0_jitter, _points

__all__ = ["IterativeGP"]

#: precond_rank=None: the best of {0, 32, 128, 512} by total time (build + solve) at N = 65536, d = 32 on the benchmark's data
#: (tools/cg_bench.py; DESIGN 3.3 "Exact GP past the factor" has the sweep).  That is NO preconditioner: those points lie far
#: apart, K is close to diagonal and CG needs 1 iteration without one and 2 with.  On smooth low-dimensional data a rank of
#: 32 - 128 pays at once (61 iterations against 4 on the tests' problem A): ask for it.
DEFAULT_PRECOND_RANK = 0
MAXITER_CAP = 1000
#: probes=None: one group of CG columns, the unit of cost of a pass (DESIGN 3.3 "Marginal likelihood by Lanczos quadrature")
DEFAULT_PROBES = 32


def lanczos_quadrature(alpha, beta):
    r""":math:`e_1^\top \log(T) e_1` for the Lanczos tridiagonal of one CG run with step lengths `alpha` (``m``) and ratios
    `beta` (the first ``m - 1`` are used): ``T[j, j] = 1 / alpha_j + beta_{j-1} / alpha_{j-1}``, ``T[j, j+1] = sqrt(beta_j) /
    alpha_j``.  ``m = 0`` (a zero probe) gives 0.  The eigenproblem goes to LAPACK's QL / QR driver: a long CG run loses
    orthogonality and its tridiagonal has clusters of near-copies of converged eigenvalues, on which the default driver
    (``stemr``) reports "did not converge"; for the quadrature the copies are harmless -- their weights add up."""
    from scipy.linalg import eigh_tridiagonal

    a = np.asarray(alpha, dtype=DTYPE)
    m = a.size
    if m == 0:
        return 0.0
    b = np.asarray(beta, dtype=DTYPE)[:m - 1]
    diag = 1.0 / a
    diag[1:] += b / a[:-1]
    if m == 1:
        return float(np.log(diag[0]))
    w, v = eigh_tridiagonal(diag, np.sqrt(b) / a[:-1], lapack_driver="stev")
    return float(np.sum(v[0] ** 2 * np.log(w)))


class _CgState(Handle):
    """Owns the gpx_cg handle of one IterativeGP; rebuilt whenever a shape or the kernel family changes."""
    _destroy = "gpx_cg_destroy"

    def __init__(self, dtype_id, kernel_id, n, d, device):
        Handle.__init__(self)
        self.key = (dtype_id, kernel_id, n, d, device)
        self.x_version = self.y_version = self.alpha_version = -1
        self.pre_key = None        # (x version, kernel parameters, s, rank, selection tol) of the preconditioner on the device
        self.rank = 0              # rows of R in use
        _lib.check(select_device(device).gpx_cg_create(ctypes.byref(self.handle), dtype_id, kernel_id, n, d))


def _native_id(K, d=None):
    kid = native_id(K, d)
    if kid is None:
        raise NotImplementedError("IterativeGP needs a built-in kernel (GaussianKernel, PeriodicKernel, GaussianARDKernel): "
                                  "plugin kernels are not supported")
    return kid


class IterativeGP(ParamsMixin):
    r"""Exact GP regression by preconditioned conjugate gradients; no n x n matrix is ever formed.

    Parameters
    ----------
    K : one of the built-in kernels (`GaussianKernel`, `PeriodicKernel`, `GaussianARDKernel`)
    x : ``(n,)`` or ``(n, d)`` input locations;  y : ``(n,)`` observations
    s : standard deviation of the observation noise, ``> 0`` (the preconditioner divides by :math:`s^2`)
    precond_rank : rows of the pivoted partial Cholesky factor behind the preconditioner, ``0 .. n``; 0 is none;
        ``None`` is 0, the best of a sweep at N = 65536 on the benchmark's nearly diagonal K -- on smooth low-dimensional data
        ask for 32 - 128, which cut the iterations many times over.  The selection stops early once no point has a
        conditional variance above ``sqrt(eps) k(0)`` (`SparseGP.greedy_inducing`'s automatic `tol`): fewer rows are then used.
    tol : relative residual :math:`\|r\| / \|b\|` at which a solve stops, ``0 < tol < 1``; ``None`` is ``sqrt(eps)``
    maxiter : iterations at most, ``>= 1``; ``None`` is ``min(n, 1000)``
    dtype : ``"float64"`` only (an fp32-product, fp64-recurrence solver is not implemented)

    There is deliberately no exact `log_lh`, and no `cov`, `sample`, pickling or `DistributedGP` counterpart here.  The
    marginal likelihood is available as a STOCHASTIC ESTIMATE -- `log_lh_estimate`, `log_lh_and_grad` and `optimize`, named
    so because the log determinant comes from Lanczos quadrature on the CG coefficients of random probes (Gardner et al.
    2018): its `info` carries the standard error, and given probes (``probes=sqrt(n) * np.eye(n)`` at rank 0 is the exact
    trace) make it deterministic.  Nothing n x n is formed for it either.
    """

    def __init__(self, K, x, y, s, precond_rank=None, tol=None, maxiter=None, dtype="float64", device=None):
        _native_id(K)
        if dtype_id(dtype) != _lib.F64:
            raise NotImplementedError("IterativeGP is float64 only (an fp32-product, fp64-recurrence solver is not implemented)")
        self.K = K
        self._x = self._y = self._s = None
        self._dtype = _lib.F64
        self._device = device
        self._dev = None
        self._version = 0          # bumped by every invalidation
        self._x_version = 0        # ... when x changes: x is uploaded again and the preconditioner rebuilt
        self._y_version = 0        # ... when y changes: only y is uploaded, R stays
        self._memoized = {}
        self._precond_rank = self._tol = self._maxiter = None
        self.x = x
        self.y = y
        self.s = s
        self.precond_rank = precond_rank
        self.tol = tol
        self.maxiter = maxiter

    # ---- invalidation: SparseGP's scheme ----
    def _invalidate(self, x=False, y=False):
        self._memoized = {}
        self._version += 1
        if x:
            self._x_version += 1
        if y:
            self._y_version += 1

    @property
    def x(self):
        return self._x

    @x.setter
    def x(self, val):
        if _changed(val, self._x):
            arr = _points("x", val, copy=True)[0]
            self._invalidate(x=True)
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
            self._invalidate(y=True)
            self._y = arr
            self._y.flags.writeable = False

    @property
    def s(self):
        return self._s

    @s.setter
    def s(self, val):
        if not (val > 0) or not np.isfinite(val):
            raise ValueError("invalid value for s: %s (the preconditioner divides by s^2: s > 0)" % val)
        if val != self._s:
            self._invalidate()
            self._s = DTYPE(val)

    @property
    def precond_rank(self):
        r"""The rank in force: the one given, or the default (0: no preconditioner)."""
        return min(self._n, DEFAULT_PRECOND_RANK) if self._precond_rank is None else self._precond_rank

    @precond_rank.setter
    def precond_rank(self, val):
        val = count_arg("precond_rank", val, 0, none_ok=True)
        if val is not None and val > self._n:
            raise ValueError("invalid value for precond_rank: %d (None, or an int in 0 .. n = %d)" % (val, self._n))
        if val != self._precond_rank:
            self._invalidate()
            self._precond_rank = val

    @property
    def tol(self):
        r"""The relative residual in force: the one given, or ``sqrt(eps)``."""
        return float(np.sqrt(dtype_eps(self._dtype))) if self._tol is None else self._tol

    @tol.setter
    def tol(self, val):
        if val is not None:
            if isinstance(val, bool) or not np.isscalar(val) or not np.isreal(val) or not (0.0 < float(val) < 1.0):
                raise ValueError("invalid value for tol: %r (None, or a relative residual 0 < tol < 1)" % (val,))
            val = float(val)
        if val != self._tol:
            self._invalidate()
            self._tol = val

    @property
    def maxiter(self):
        r"""The iteration limit in force: the one given, or ``min(n, 1000)``."""
        return min(self._n, MAXITER_CAP) if self._maxiter is None else self._maxiter

    @maxiter.setter
    def maxiter(self, val):
        val = count_arg("maxiter", val, 1, none_ok=True)
        if val != self._maxiter:
            self._invalidate()
            self._maxiter = val

    @property
    def _n(self):
        return self._x.shape[0]

    @property
    def _d(self):
        return 1 if self._x.ndim == 1 else self._x.shape[1]

    def __reduce_ex__(self, protocol):
        raise NotImplementedError("IterativeGP is not copied or pickled: its state is a device handle; make a new one from (K, x, y, s)")

    # ---- device plumbing ----
    def _state(self):
        """The handle with the current x and y on the device and the preconditioner of the current parameters."""
        if self._y.shape[0] != self._n:
            raise ValueError("invalid shape for y: %s (x has %d rows)" % (str(self._y.shape), self._n))
        if self._precond_rank is not None and self._precond_rank > self._n:
            raise ValueError("invalid value for precond_rank: %d (x has %d rows now)" % (self._precond_rank, self._n))
        key = (self._dtype, _native_id(self.K, self._d), self._n, self._d, self._device)
        if self._dev is None or self._dev.key != key:
            if self._dev is not None:
                self._dev.close()
            self._dev = _CgState(*key)
        st = self._dev
        lib = _lib.load()
        if st.x_version != self._x_version or st.y_version != self._y_version:
            xs = _lib.dptr(np.ascontiguousarray(self._x, dtype=DTYPE)) if st.x_version != self._x_version else None
            ys = _lib.dptr(np.ascontiguousarray(self._y, dtype=DTYPE)) if st.y_version != self._y_version else None
            _lib.check(lib.gpx_cg_set_data(st.handle, xs, ys))
            st.x_version, st.y_version = self._x_version, self._y_version
            st.alpha_version = -1
        p = np.ascontiguousarray(self.K.params, dtype=DTYPE)
        rank = self.precond_rank
        sel_tol = _k0_jitter(self.K, self._x[:1], self._dtype) if rank > 0 else 0.0
        pre_key = (self._x_version, tuple(p), float(self._s), rank, sel_tol)
        if st.pre_key != pre_key:
            count = ctypes.c_int64(0)
            st.pre_key = None
            _lib.check(lib.gpx_cg_precond(st.handle, _lib.dptr(p), float(self._s), rank, sel_tol, ctypes.byref(count)))
            st.pre_key, st.rank = pre_key, int(count.value)
            st.alpha_version = -1
        return st

    def _solve(self, B):
        """One device solve: B None (the handle's y) or ``(S, n)``.  ``(X, info)``."""
        st = self._state()
        S = 1 if B is None else B.shape[0]
        X = np.empty((S, self._n), dtype=DTYPE)
        iters = np.zeros(S, dtype=np.int32)
        relres = np.empty(S, dtype=DTYPE)
        p = np.ascontiguousarray(self.K.params, dtype=DTYPE)
        _lib.check(_lib.load().gpx_cg_solve(st.handle, _lib.dptr(p), float(self._s), None if B is None else _lib.dptr(B), S, self.tol,
                                            self.maxiter, _lib.dptr(X), iters.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                            _lib.dptr(relres)))
        if B is None:
            st.alpha_version = self._version
        # (a column frozen by rr <= tol^2 bb reports sqrt(rr / bb): within a rounding of tol)
        converged = (iters >= 0) & (relres <= self.tol * (1.0 + 4.0 * np.finfo(DTYPE).eps))
        info = {"iterations": iters.astype(np.int64), "relres": relres, "converged": converged, "rank": st.rank}
        return X, info

    def _solve_y(self):
        st = self._dev
        if "alpha" not in self._memoized or st is None or st.alpha_version != self._version:
            X, info = self._solve(None)
            self._memoized["alpha"] = (X[0], info)
            if not info["converged"][0]:
                warnings.warn("IterativeGP: the solve for y stopped at relative residual %.3e (tol %.3e) after maxiter = %d iterations; "
                              "the iterate reached is returned" % (info["relres"][0], self.tol, self.maxiter), RuntimeWarning, stacklevel=3)
        return self._memoized["alpha"]

    @property
    def inv_Kxx_y(self):
        r""":math:`(K_{xx} + s^2 I)^{-1} y`, ``(n,)``, memoized.  When the solve does not reach `tol` within `maxiter` it warns
        once per fit (``RuntimeWarning``) and returns the iterate reached: `solve_info` says how far it got."""
        return self._solve_y()[0]

    @property
    def solve_info(self):
        r"""The record of the `inv_Kxx_y` solve: ``iterations``, ``relres``, ``converged`` (arrays of one entry) and ``rank``."""
        return dict(self._solve_y()[1])

    def solve(self, B):
        r"""``(X, info)`` with :math:`X = B (K_{xx} + s^2 I)^{-1}` row by row, for `B` of shape ``(n,)`` or ``(S, n)``; `X` has
        the shape of `B`.  ``info``: per column ``iterations`` (the iteration at which the column reached `tol`, `maxiter`
        when it did not; negative when the recurrence lost positive definiteness to rounding there), ``relres``
        :math:`\|r\| / \|b\|` of the recurrence and ``converged``, plus ``rank`` (rows of R in use).  A column that has
        converged is frozen: its result does not depend on its batch companions.  Not converged is not an error."""
        arr = np.ascontiguousarray(B, dtype=DTYPE)
        if arr.ndim not in (1, 2) or arr.shape[-1] != self._n or arr.shape[0] < 1:
            raise ValueError("invalid shape for B: %s (n = %d: (n,) or (S, n))" % (str(arr.shape), self._n))
        check_finite(arr)
        X, info = self._solve(arr.reshape(-1, self._n))
        return X.reshape(arr.shape), info

    # ---- predictions ----
    def _xo(self, xo):
        return points_arg("xo", xo, self._d)

    def mean(self, xo):
        r"""Predictive mean :math:`k(x^*, x) (K_{xx} + s^2 I)^{-1} y`, ``(m,)``: one fused device pass with `inv_Kxx_y`."""
        xo, m = self._xo(xo)
        self._solve_y()
        out = np.empty(m, dtype=DTYPE)
        p = np.ascontiguousarray(self.K.params, dtype=DTYPE)
        _lib.check(_lib.load().gpx_cg_mean(self._dev.handle, _lib.dptr(p), _lib.dptr(xo), m, _lib.dptr(out)))
        return out

    def var(self, xo, noise=False):
        r"""Predictive variance :math:`k(x^*, x^*) - k(x^*, x) (K_{xx} + s^2 I)^{-1} k(x, x^*)`, ``(m,)``: one batched solve per
        32 test points, so ``m / 32`` solves -- meant for hundreds of points, not millions.  ``noise=True`` adds
        :math:`s^2`.  Not clamped at zero.  Warns (``RuntimeWarning``) when a column did not reach `tol`."""
        xo, m = self._xo(xo)
        st = self._state()
        out = np.empty(m, dtype=DTYPE)
        worst = ctypes.c_double(0.0)
        p = np.ascontiguousarray(self.K.params, dtype=DTYPE)
        _lib.check(_lib.load().gpx_cg_var(st.handle, _lib.dptr(p), float(self._s), _lib.dptr(xo), m, self.tol, self.maxiter,
                                          _lib.dptr(out), ctypes.byref(worst)))
        if not worst.value <= self.tol * (1.0 + 4.0 * np.finfo(DTYPE).eps):
            warnings.warn("IterativeGP.var: a solve stopped at relative residual %.3e (tol %.3e) after maxiter = %d iterations"
                          % (worst.value, self.tol, self.maxiter), RuntimeWarning, stacklevel=2)
        if noise:
            out += self._s ** 2
        return out

    def predict(self, xo, noise=False):
        r"""``(mean(xo), var(xo, noise))``."""
        xo, _ = self._xo(xo)
        return self.mean(xo), self.var(xo, noise=noise)

    # ---- the marginal likelihood: stochastic Lanczos quadrature ----
    def _probes_arg(self, probes, seed):
        """(Z or None, T, seed) of a `probes` argument, checked before the library is touched."""
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not (0 <= int(seed) < 2 ** 64):
            raise ValueError("invalid value for seed: %r (an int in 0 .. 2^64 - 1)" % (seed,))
        if probes is None:
            return None, DEFAULT_PROBES, int(seed)
        if isinstance(probes, np.ndarray) or isinstance(probes, (list, tuple)):
            Z = np.ascontiguousarray(probes, dtype=DTYPE)
            if Z.ndim != 2 or Z.shape[1] != self._n or Z.shape[0] < 1:
                raise ValueError("invalid shape for probes: %s (n = %d: None, an int >= 1 or a (T, n) array)" % (str(Z.shape), self._n))
            check_finite(Z)
            return Z, Z.shape[0], int(seed)
        return None, count_arg("probes", probes, 1), int(seed)

    def probes(self, T, seed=0):
        r"""The `T` probe rows the device generates for `seed`, ``(T, n)``: :math:`z \sim N(0, P)` with the preconditioner
        :math:`P = R^\top R + s^2 I` of the current parameters -- ``z = g1 R + s g2`` from the counter-based normal sequence
        (``gpx_d_randn``; `g2` is stream 4, `g1` stream 5), and ``z = g2`` at rank 0 (:math:`P = I`).  Row `t` depends on
        ``(seed, t)`` alone: fewer probes are a prefix of more."""
        _, T, seed = self._probes_arg(count_arg("T", T, 1), seed)
        st = self._state()
        out = np.empty((T, self._n), dtype=DTYPE)
        _lib.check(_lib.load().gpx_cg_probes(st.handle, T, seed, _lib.dptr(out)))
        return out

    def _lh(self, probes, seed, want_grad):
        """One device pass (memoized per argument set): the record `log_lh_estimate` and `log_lh_and_grad` are read from."""
        Z, T, seed = self._probes_arg(probes, seed)
        key = ("lh", T if Z is None else Z.tobytes(), seed)
        have = self._memoized.get(key)
        if have is not None and (have["grad"] is not None or not want_grad):
            return have
        alpha, fit = self._solve_y()                  # (memoized; warns once when y's own solve stopped at maxiter)
        st = self._state()
        n, maxiter = self._n, self.maxiter
        npar = self.K.params.size
        rho0, relres = np.empty(T, dtype=DTYPE), np.empty(T, dtype=DTYPE)
        iters = np.zeros(T, dtype=np.int32)
        coef = np.empty((T, maxiter, 2), dtype=DTYPE)
        scalars = np.empty(2, dtype=DTYPE)
        sums, grad = np.empty(max(4, self._d + 2), dtype=DTYPE), np.empty(npar + 1, dtype=DTYPE)
        p = np.ascontiguousarray(self.K.params, dtype=DTYPE)
        _lib.check(_lib.load().gpx_cg_lh(st.handle, _lib.dptr(p), float(self._s), None if Z is None else _lib.dptr(Z), T, seed, self.tol,
                                         maxiter, 1 if want_grad else 0, _lib.dptr(rho0), iters.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                         _lib.dptr(relres), _lib.dptr(coef), _lib.dptr(scalars), _lib.dptr(sums), _lib.dptr(grad)))
        st.alpha_version = self._version
        its = iters.astype(np.int64)
        lost = its < 0                                # positive definiteness lost to rounding in that column
        quad = np.array([np.nan if lost[t] else rho0[t] * lanczos_quadrature(coef[t, :its[t], 0], coef[t, :its[t], 1]) for t in range(T)])
        converged = ~lost & (relres <= self.tol * (1.0 + 4.0 * np.finfo(DTYPE).eps))
        logdet = float(scalars[0] + quad.mean()) if not lost.any() else np.inf
        value = -0.5 * float(scalars[1]) - 0.5 * logdet - 0.5 * n * np.log(2.0 * np.pi)
        if not converged[~lost].all():
            warnings.warn("IterativeGP: %d of %d probe solves stopped above tol %.3e after maxiter = %d iterations (worst relative "
                          "residual %.3e); the quadrature of the shorter Lanczos runs is returned"
                          % (int((~converged & ~lost).sum()), T, self.tol, maxiter, float(relres[~lost].max())), RuntimeWarning, stacklevel=3)
        if want_grad and lost.any():
            grad = np.full(npar + 1, np.nan)
        info = {"logdet": logdet, "logdet_precond": float(scalars[0]), "quad": quad,
                "stderr": float(quad.std(ddof=1) / np.sqrt(T)) if T > 1 else float("nan"), "fit": -0.5 * float(scalars[1]),
                "iterations": its, "relres": relres, "converged": converged, "rank": st.rank}
        rec = {"value": float(value), "grad": grad if want_grad else None, "info": info}
        self._memoized[key] = rec
        return rec

    def log_lh_estimate(self, probes=None, seed=0, return_info=False):
        r"""A stochastic estimate of the log marginal likelihood,

        .. math:: -\tfrac12 y^\top \alpha - \tfrac12 \Big(\log\det P + \tfrac1T \sum_t \rho_t\, e_1^\top \log(T_t)\, e_1\Big) - \tfrac n2 \log 2\pi

        with :math:`T_t` the Lanczos tridiagonal of probe `t` read off its CG coefficients (``T[j, j] = 1 / a_j + b_{j-1} /
        a_{j-1}``, ``T[j, j+1] = sqrt(b_j) / a_j``) and :math:`\rho_t = z_t^\top P^{-1} z_t`; the eigenproblem of the small
        tridiagonals is the host's (``scipy.linalg.eigh_tridiagonal``).  `probes`: ``None`` (32: one group of columns, the unit
        of cost), an int ``>= 1`` (that many, generated on the device from `seed`: `probes`), or a ``(T, n)`` array used as
        given -- the caller answers for its distribution: the rows' second moment ``Z.T @ Z / T`` must be `P` in expectation
        (at rank 0 the identity; ``sqrt(n) * np.eye(n)`` has it exactly, and the estimate is then the exact trace).  The same arguments give the same bits, and the result is memoized.

        ``return_info=True``: ``(value, info)`` with ``logdet``, ``logdet_precond``, ``quad`` (the `T` per-probe terms),
        ``stderr`` (their standard error: that of ``logdet``), ``fit`` (:math:`-y^\top\alpha / 2`), per probe
        ``iterations`` / ``relres`` / ``converged``, and ``rank``.  A probe column whose recurrence lost positive
        definiteness (negative count) makes the value ``-inf`` without raising; a column that stopped at `maxiter` warns
        (``RuntimeWarning``) and the value is still returned: the quadrature of a shorter Lanczos run is still a quadrature."""
        rec = self._lh(probes, seed, False)
        return (rec["value"], dict(rec["info"])) if return_info else rec["value"]

    def log_lh_and_grad(self, probes=None, seed=0):
        r"""``(value, grad)``: `log_lh_estimate` and the estimate of its gradient over `params`, (kernel parameters..., s),

        .. math:: \tfrac12 \alpha^\top \partial K \alpha - \tfrac12 \tfrac1T \sum_t w_t^\top \partial K\, \tilde z_t,
                  \qquad w_t = (K + s^2 I)^{-1} z_t, \quad \tilde z_t = P^{-1} z_t

        which uses :math:`E[\tilde z z^\top] = I` for :math:`z \sim N(0, P)`.  Both contractions run in one fused tile
        reduction per group of 32 probes that forms the low-rank coefficients inside the tile (``gpx_d_lowrank_reduce``): no
        n x n matrix exists.  The noise component comes from the reduction's trace slot.  ``NaN`` gradients (and ``-inf``)
        when a probe column lost positive definiteness."""
        rec = self._lh(probes, seed, True)
        return rec["value"], np.array(rec["grad"], copy=True)

    def optimize(self, maxiter=50, bounds=None, probes=None, seed=0):
        r"""Maximise `log_lh_estimate` over `params` (all positive) with scipy's L-BFGS-B in log-parameters; one
        `log_lh_and_grad` call per evaluation, all with the same `probes` and `seed` (common random numbers: the objective is
        one smooth function of the parameters, not a fresh draw per evaluation).  With generated probes the gradient is that of
        the EXPECTATION over probes, not of the fixed-probe estimate (the probes' distribution moves with the preconditioner,
        and its derivative is not taken), so the line search sees a slightly inconsistent pair; with given probes at rank 0
        the two agree up to the solves' tolerance.  `bounds`: ``None``, or one ``(lo, hi)`` pair per parameter in the natural
        scale.  The object is left at the best parameters evaluated.  Returns a dict: ``params``, ``log_lh_estimate``,
        ``evaluations``, ``nit``, ``success``, ``message``."""
        from scipy.optimize import minimize

        self._probes_arg(probes, seed)
        npar = self.params.size
        if bounds is not None:
            bounds = list(bounds)
            if len(bounds) != npar:
                raise ValueError("bounds: one (lo, hi) pair per parameter (%d), got %d" % (npar, len(bounds)))
            bounds = [tuple(None if b is None else float(np.log(b)) for b in pair) for pair in bounds]
        best = {"value": -np.inf, "params": self.params}
        state = {"worst": None, "evaluations": 0}

        def negative(u):
            self.params = np.exp(u)
            state["evaluations"] += 1
            val, grad = self.log_lh_and_grad(probes=probes, seed=seed)
            if not (np.isfinite(val) and np.all(np.isfinite(grad))):
                ref = state["worst"] if state["worst"] is not None else 0.0
                return abs(ref) * 10.0 + 1e10, np.zeros_like(u)
            if val > best["value"]:
                best["value"], best["params"] = float(val), self.params
            state["worst"] = -val if state["worst"] is None else max(state["worst"], -val)
            return -float(val), -grad * np.exp(u)                 # d/d log theta = theta d/d theta

        res = minimize(negative, np.log(self.params), jac=True, method="L-BFGS-B", bounds=bounds, options={"maxiter": int(maxiter)})
        self.params = best["params"]
        found = bool(np.isfinite(best["value"]))
        msg = res.message.decode() if isinstance(res.message, bytes) else str(res.message)
        return dict(params=self.params, log_lh_estimate=DTYPE(best["value"]), evaluations=state["evaluations"], nit=int(res.nit),
                    success=found and bool(res.success), message=msg if found else "no trial point had a finite estimate")

    def timing(self):
        """Milliseconds (HIP events on the handle's stream): ``precond`` the last preconditioner build; of the last solve
        (`inv_Kxx_y`, `solve`, `var` or an estimate's pass): ``product`` the products with K, ``apply`` the preconditioner applies, ``vector`` the
        dots and updates, ``total``, and ``read`` the per-iteration status reads."""
        return timing("gpx_cg_last_timing", self._state().handle, ("precond", "product", "apply", "vector", "total", "read"))

    @property
    def device_bytes(self):
        """Bytes of device memory the handle owns now."""
        out = ctypes.c_size_t(0)
        _lib.check(_lib.load().gpx_cg_device_bytes(self._state().handle, ctypes.byref(out)))
        return int(out.value)
