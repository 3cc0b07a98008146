"""DistributedGP -- the drop-in `GP` interface on the multi-GPU fit.

At the sizes the multi-GPU path exists for (K and its factor no longer fit one GPU's HBM), a user gets the same
object as `gp.GP` -- ``log_lh``, ``lh``, ``inv_Kxx_y``, ``mean(xo)``, ``cov(xo)``, ``var(xo)``, ``predict(xo)``, the setters, ``params`` /
``set_param`` and the memoisation rules -- on top of one rank's `multi_gpu.NativeDistributedGP` handle:

    g = gp.DistributedGP(gp.GaussianKernel(1.0, 0.5), x, y, s=1.0, dist=dist)      # backend="rccl"
    g.log_lh, g.inv_Kxx_y, g.mean(xo), g.cov(xo)

Every rank builds the same object with the same data and calls the same members in the same order: a fit, a mean
and a cov are collective.  The factor never leaves the ranks' HBM, so what needs an n x n host copy (`Kxx`, `Lxx`,
`inv_Kxx`, the derivative stack, `dm_dtheta`), leave-one-out, the input-space gradients, growing and shrinking the fit and joint samples (`loo`, `inv_Kxx_diag`, `dloo_dtheta`, `dmean_dx`, `dvar_dx`,
`predict_grad`, `extend`, `remove`, `sample`, `sample_paths`: not implemented over the distributed factor) and what would have to carry a handle or a communicator to another
process (`save_fitted`, copy, pickle) raises NotImplementedError: `GP` has them.
"""
import numpy as np

from . import _lib, multi_gpu
from ._facade import FAMILIES, native_id
from .gp import GP, DTYPE, memoprop

__all__ = ["DistributedGP"]


def _unsupported(name, why="it needs an n x n host copy of a matrix that stays distributed, or a handle and communicator "
                           "that do not travel"):
    msg = "DistributedGP.%s is not available (%s): use gp.GP for it" % (name, why)

    def f(*args, **kwargs):
        raise NotImplementedError(msg)
    f.__name__ = name
    f.__doc__ = msg
    return f


def _native_kernel_id(K):
    kid = native_id(K)
    if kid is None:
        raise TypeError("DistributedGP needs a built-in kernel (GaussianKernel or PeriodicKernel); %s is a Python "
                        "kernel plugin, which gp.GP supports on one GPU" % type(K).__name__)
    if not FAMILIES[kid].multi_gpu:
        raise NotImplementedError("DistributedGP does not support %s: the multi-GPU fit knows GaussianKernel and "
                                  "PeriodicKernel only; gp.GP has the ARD family on one GPU" % type(K).__name__)
    return kid


class DistributedGP(GP):
    r"""Gaussian process regression over several GPUs (one rank per process; `GP`'s interface).

    Parameters
    ----------
    K : GaussianKernel or PeriodicKernel
        A built-in kernel (Python kernel plugins are refused).
    x, y, s : as for `GP`.
    dist : torch.distributed, or None
        The control plane (a CPU group is used for it); None: one rank.
    callbacks : object, optional
        backend="callbacks" only: the host-collective transport (see `multi_gpu.NativeDistributedGP`); default:
        `multi_gpu.GlooCallbacks(dist)` when there is more than one rank.
    backend : "rccl" or "callbacks"
    nb : int, optional
        Block-column width (default: `multi_gpu.default_nb`).
    device : int, optional
        This rank's GPU (default: the current device).
    dtype : "float64" or "float32"
    """

    def __init__(self, K, x, y, s=0, dist=None, callbacks=None, backend="rccl", nb=None, device=None,
                 dtype="float64"):
        _native_kernel_id(K)
        if backend not in ("rccl", "callbacks"):
            raise ValueError("backend must be 'rccl' or 'callbacks'")
        self._mg = None                # multi_gpu.NativeDistributedGP, created at the first collective
        self._mg_key = None
        self._mg_data_version = -1
        self._mg_fit_version = -1
        self._dist, self._backend, self._nb, self._callbacks = dist, backend, nb, callbacks
        GP.__init__(self, K, x, y, s=s, dtype=dtype, device=device)

    # ---- inputs: GP's setters, and a new n or d is a change (GP's element-wise comparison does not broadcast across
    # it); the next collective member re-creates the handle ----
    @GP.x.setter
    def x(self, val):
        if self._x is not None and np.shape(val) != self._x.shape:
            self._x = None
        GP.x.fset(self, val)

    @GP.y.setter
    def y(self, val):
        if self._y is not None and np.shape(val) != self._y.shape:
            self._y = None
        GP.y.fset(self, val)

    # ---- the rank's handle ----
    def _handle(self):
        """This rank's NativeDistributedGP with the current data: re-created (taking over the communicator, never a
        second ncclCommInitRank) when n, d, the kernel family or the dtype change."""
        kid = _native_kernel_id(self.K)
        key = (self._dtype, kid, self._n, self._d)
        if self._mg is None or self._mg_key != key:
            old, self._mg = self._mg, None
            adopt = old if (old is not None and self._backend == "rccl") else None
            if old is not None and adopt is None:
                old.close()                          # (host callbacks: nothing to take over)
            cb = None
            if self._backend == "callbacks":
                if self._callbacks is None and self._dist is not None and self._dist.get_world_size() > 1:
                    self._callbacks = multi_gpu.GlooCallbacks(self._dist)
                cb = self._callbacks
            device = self._device
            if device is None:
                import ctypes
                cur = ctypes.c_int(0)
                _lib.check(_lib.load().gpx_get_device(ctypes.byref(cur)))
                device = cur.value
            try:
                new = multi_gpu.NativeDistributedGP(self._n, self._d, dtype_id=self._dtype, kernel_id=kid, nb=self._nb,
                                                    dist=self._dist, backend=self._backend, device=device,
                                                    callbacks=cb, adopt_from=adopt)
            except Exception:
                self._mg = adopt                     # (a failed take-over leaves the communicator where it was)
                raise
            if adopt is not None:
                adopt.close()
            self._mg, self._mg_key = new, key
            self._mg_data_version = self._mg_fit_version = -1
        mg = self._mg
        if self._mg_data_version != self._data_version:
            mg.set_data(self._x, self._y)
            self._mg_data_version = self._data_version
            self._mg_fit_version = -1
        return mg

    def _fit(self):
        """Make the distributed state current (collective): build, factor, solve; `.info` as `GP`'s device state."""
        mg = self._handle()
        if self._mg_fit_version != self._version:
            mg.fit(np.ascontiguousarray(self.K.params, dtype=DTYPE), float(self._s))
            self._mg_fit_version = self._version
        return mg

    def close(self):
        """Release this rank's handle (device memory, streams, communicator)."""
        if self._mg is not None:
            self._mg.close()
            self._mg = None
            self._mg_key = None

    @property
    def native(self):
        """This rank's `multi_gpu.NativeDistributedGP` (created on first use)."""
        return self._handle()

    # ---- the members that work distributed ----
    @memoprop
    def log_lh(self):
        r"""Log marginal likelihood (collective); ``-inf`` on every rank when `Kxx` is not positive definite."""
        mg = self._fit()
        if mg.info != 0:
            return -np.inf
        return DTYPE(mg.log_lh)

    @memoprop
    def inv_Kxx_y(self):
        r""":math:`K_{xx}^{-1} y` (collective; replicated on every rank)."""
        return self._fit_pd().alpha

    def mean(self, xo):
        r"""Predictive mean at xo (collective; every rank gets all of it)."""
        xo, m = self._xo(xo)                         # a bad shape raises before any collective
        mg = self._fit_pd()
        return mg.mean(np.ascontiguousarray(self.K.params, dtype=DTYPE), xo.reshape(m, self._d))

    def cov(self, xo):
        r"""Predictive covariance at xo, ``(m, m)`` on every rank (collective: gpx_mg_cov, the factor stays
        distributed).  Ranks that disagree on xo raise `multi_gpu.RankMismatchError` together."""
        xo, m = self._xo(xo)
        mg = self._fit_pd()
        return mg.cov(np.ascontiguousarray(self.K.params, dtype=DTYPE), xo.reshape(m, self._d))

    def var(self, xo, noise=False, chunk_rows=0):
        r"""Predictive variance at xo, ``(m,)`` on every rank (collective: gpx_mg_var, row chunks of xo over the
        distributed factor; any m).  ``noise=True`` adds :math:`s^2`.  Not clamped at zero, as `GP.var`.  Ranks that
        disagree on xo or chunk_rows raise `multi_gpu.RankMismatchError` together."""
        xo, m = self._xo(xo)
        mg = self._fit_pd()
        out = mg.var(np.ascontiguousarray(self.K.params, dtype=DTYPE), xo.reshape(m, self._d), chunk_rows=chunk_rows)
        if noise:
            out += self._s ** 2
        return out

    def predict(self, xo, noise=False):
        r"""``(mean(xo), var(xo, noise))`` (two collectives)."""
        xo, _ = self._xo(xo)
        return self.mean(xo), self.var(xo, noise=noise)

    def fit_timing(self):
        """This rank's stage times of the last fit, ms (`NativeDistributedGP.timing`)."""
        return self._fit().timing()

    # ---- what stays with GP ----
    Kxx = property(_unsupported("Kxx"))
    Kxx_J = property(_unsupported("Kxx_J"))
    Kxx_H = property(_unsupported("Kxx_H"))
    Lxx = property(_unsupported("Lxx"))
    inv_Kxx = property(_unsupported("inv_Kxx"))
    dloglh_dtheta = property(_unsupported("dloglh_dtheta"))
    dlh_dtheta = property(_unsupported("dlh_dtheta"))
    d2lh_dtheta2 = property(_unsupported("d2lh_dtheta2"))
    d2loglh_dtheta2 = property(_unsupported("d2loglh_dtheta2"))
    dm_dtheta = _unsupported("dm_dtheta")
    _NO_LOO = "leave-one-out over the distributed factor is not implemented; one GPU has it"
    inv_Kxx_diag = property(_unsupported("inv_Kxx_diag", _NO_LOO))
    loo_mean = property(_unsupported("loo_mean", _NO_LOO))
    loo_var = property(_unsupported("loo_var", _NO_LOO))
    loo_log_lh = property(_unsupported("loo_log_lh", _NO_LOO))
    loo = _unsupported("loo", _NO_LOO)
    dloo_dtheta = property(_unsupported("dloo_dtheta", _NO_LOO))
    _NO_XGRAD = "input-space gradients over the distributed factor are not implemented; one GPU has them"
    dmean_dx = _unsupported("dmean_dx", _NO_XGRAD)
    dvar_dx = _unsupported("dvar_dx", _NO_XGRAD)
    predict_grad = _unsupported("predict_grad", _NO_XGRAD)
    extend = _unsupported("extend", "appending rows to the distributed factor is not implemented; one GPU has it")
    remove = _unsupported("remove", "deleting rows of the distributed factor is not implemented; one GPU has it")
    sample = _unsupported("sample", "joint samples over the distributed factor are not implemented; one GPU has them")
    sample_paths = _unsupported("sample_paths", "posterior paths over the distributed factor are not implemented; one GPU has them")
    save_fitted = _unsupported("save_fitted")
    load_fitted = classmethod(_unsupported("load_fitted"))
    _state = _unsupported("_state")
    copy = _unsupported("copy")
    __copy__ = _unsupported("__copy__")
    __deepcopy__ = _unsupported("__deepcopy__")
    __getstate__ = _unsupported("__getstate__")
    __setstate__ = _unsupported("__setstate__")
    __reduce__ = _unsupported("__reduce__")
    __reduce_ex__ = _unsupported("__reduce_ex__")
