r"""PosteriorPaths -- draws of the posterior FUNCTION, to be evaluated at any number of points (`GP.sample_paths`).

Pathwise conditioning (Matheron's rule; Wilson et al. 2020): a draw is a function,

    f_s(a) = phi(a) . Theta_s + sum_j k(a, x_j) V[s, j],      V_s = alpha - Kxx^-1 (Phi(x) Theta_s + s E_s)

-- a random-feature draw of the prior plus an exact, data-dependent update -- stored as one weight vector per path in HBM.
Evaluating `size` paths at `m` points costs O(m n) kernel evaluations and O(m n size) multiply-adds; nothing ``(m, m)`` is
ever formed, so a Thompson-sampling round can draw once and then optimise the draw over tens of thousands of candidates.

The whole object is a pure function of ``(seed, size, features)`` and the fitted GP.  With `z(seed, stream, e)` the
counter-based sequence of ``gpx_d_randn`` (include/gpx.h; stream 0 stays `GP.sample`'s), `p` the points `x` (Gaussian) or
`x / w` (ARD), ``(h_v, w_v)`` the isotropic constants ``(h, w)`` or ``(h / sqrt(wbar), 1)``, ``k0 = h_v^2 / (w_v sqrt(2 pi))``
and `F` = `features`:

    Omega[f, k] = z(seed, 1, f d + k) / w_v          spectral frequencies (float64 for both dtypes)
    Theta[s, q] = z(seed, 2, s 2F + q)               feature weights
    E[s, j]     = z(seed, 3, s n + j)                the observation-noise draw
    phi(a)      = sqrt(k0 / F) [cos(Omega a); sin(Omega a)]

Row `s` of `Theta` and `E` depends on `s` alone: the random inputs of ``size=3`` are a prefix of those of ``size=9``.
The approximation lies in the prior only -- its covariance error is ``O(k0 / sqrt(F))`` -- the data update is exact.
The draws are of the LATENT function: observation noise is not added to the values.  Memory held: ``size x n`` weights,
``size x 2F`` feature weights, ``F x d`` frequencies and a copy of the ``n x d`` points, all on the device.

A path is differentiable in its input, and the derivative is as cheap as the value -- with `p` the view's points,

    d f_s / d a_k (a) = sqrt(k0 / F) sum_f Omega[f, k] (Theta[s, F + f] cos(Omega_f . a) - Theta[s, f] sin(Omega_f . a))
                        - 1 / w_v^2 sum_j V[s, j] (a_k - p_jk) k(a, p_j)

(ARD: on ``a / w``, component `k` divided by ``w_k``) -- so a draw can be maximised by a gradient-based multi-start optimiser
instead of central differences: `PosteriorPaths.grad` and `PosteriorPaths.value_and_grad` form every kernel value once per
group of paths and window of dimensions, where ``2 d + 1`` calls of the paths form it ``2 d + 1`` times.

Out of scope: second derivatives, the periodic family (an exact Fourier-series prior exists for it), plugin kernels,
`DistributedGP`, and persistence -- a paths object is regenerated from its seed, not copied or pickled.
"""
import numpy as np

from . import _lib
from ._facade import DTYPE, Handle, chunk_arg, points_arg, timing

__all__ = ["PosteriorPaths"]


class PosteriorPaths(Handle):
    """`size` posterior function draws of a fitted `GP` (made by `GP.sample_paths`); call it with test points.

    Attributes: ``size``, ``features``, ``seed``, ``n``, ``d``.  The object owns its device state and does not refer to the
    `GP` again: the GP may be modified, refitted or deleted.  `close` releases the device state now (`__del__` does it
    otherwise)."""
    _pointer, _destroy = "_handle", "gpx_paths_destroy"

    def __init__(self, handle, size, features, seed, n, d, ndim):
        Handle.__init__(self, ptr=handle)
        self.size, self.features, self.seed, self.n, self.d = size, features, seed, n, d
        self._ndim = ndim              # of the GP's x: 1 -> xo is (m,), 2 -> (m, d)

    def _checked(self, xo, chunk_rows):
        """`xo` as a contiguous float64 array and its number of points, after the refusals `__call__`, `grad` and
        `value_and_grad` share -- every one of them comes before the library is touched."""
        xo, m = points_arg("xo", xo, self.d, self._ndim)
        chunk_arg("chunk_rows", chunk_rows, strict=True)
        if not self._handle:
            raise ValueError("the paths have been closed")
        return xo, m

    def __call__(self, xo, chunk_rows=0):
        """The draws at `xo` (``(m,)`` for 1-D inputs or ``(m, d)``): ``(size, m)`` float64.  ``chunk_rows``: test points per
        device chunk, 0 (automatic) or a multiple of 128."""
        xo, m = self._checked(xo, chunk_rows)
        out = np.empty((self.size, m), dtype=DTYPE)
        _lib.check(_lib.load().gpx_paths_eval(self._handle, _lib.dptr(xo), m, int(chunk_rows), _lib.dptr(out)))
        return out

    def grad(self, xo, chunk_rows=0):
        """The gradients of the draws with respect to the input at `xo`: ``(size,) + xo.shape`` float64 -- ``(size, m)`` for
        1-D inputs, ``(size, m, d)`` otherwise; ``[s, i, k]`` is ``d f_s / d xo_ik``.  `xo` and ``chunk_rows`` as for a call."""
        xo, m = self._checked(xo, chunk_rows)
        grad = np.empty((self.size,) + xo.shape, dtype=DTYPE)
        _lib.check(_lib.load().gpx_paths_grad(self._handle, _lib.dptr(xo), m, int(chunk_rows), None, _lib.dptr(grad)))
        return grad

    def value_and_grad(self, xo, chunk_rows=0):
        """``(values (size, m), grad)``: what a call and `grad` return for the same arguments, bit for bit, from one upload of
        the points -- what a gradient-based optimiser asks for at every step."""
        xo, m = self._checked(xo, chunk_rows)
        values, grad = np.empty((self.size, m), dtype=DTYPE), np.empty((self.size,) + xo.shape, dtype=DTYPE)
        _lib.check(_lib.load().gpx_paths_grad(self._handle, _lib.dptr(xo), m, int(chunk_rows), _lib.dptr(values), _lib.dptr(grad)))
        return values, grad

    def state(self):
        """Diagnostic: ``(Omega (F, d), Theta (size, 2F), V (size, n))`` as float64 host copies (``gpx_paths_get``; the tests pin
        the definition with it)."""
        if not self._handle:
            raise ValueError("the paths have been closed")
        omega = np.empty((self.features, self.d), dtype=DTYPE)
        theta = np.empty((self.size, 2 * self.features), dtype=DTYPE)
        V = np.empty((self.size, self.n), dtype=DTYPE)
        _lib.check(_lib.load().gpx_paths_get(self._handle, _lib.dptr(omega), _lib.dptr(theta), _lib.dptr(V)))
        return omega, theta, V

    def create_timing(self):
        """Diagnostic (tools/paths_probe.py): milliseconds the creation took on the device -- features + products, the two
        sweeps, the rest, total."""
        if not self._handle:
            raise ValueError("the paths have been closed")
        return timing("gpx_debug_paths_timing", self._handle, ("features_products", "sweeps", "rest", "total"))

    def _no_copy(self, *args, **kwargs):
        raise NotImplementedError("PosteriorPaths holds device state and is not copied or pickled: regenerate it from the seed, "
                                  "gp.sample_paths(%d, seed=%d, features=%d)" % (self.size, self.seed, self.features))

    __copy__ = __deepcopy__ = __reduce_ex__ = __getstate__ = _no_copy
