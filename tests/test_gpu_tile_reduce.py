"""GPU tests of the shared tile walk of the two hyper-parameter gradients (csrc/gpx_kmat.hip: tile_reduce_kernel<T, FORM>,
tile_reduce_ard_kernel<T, DMAX, FORM>): GP.dloglh_dtheta (TILE_ML) and GP.dloo_dtheta (TILE_LOO) on ONE fitted handle at the sizes
where a walk over 64 x 64 tiles of a lower triangle can go wrong -- N = 1 and 63 (one partial tile), 64 (exactly one tile),
65 (the first off-diagonal tile, one row and one column of it), 129 (a 3 x 3 tile triangle with a ragged edge) -- for the
Gaussian family (d = 3), the periodic family (d = 1) and the ARD family at d = 9 (DMAX = 16: zero padding past d).

Nothing here is a new yardstick.  The marginal-likelihood gradient is checked as
tests/test_gpu_ard.py::test_gradient_against_the_closed_form_from_the_oracle checks it: the closed form 1/2 sum (alpha alpha^T -
K^-1) o dK from the oracle's inv_Kxx and inv_Kxx_y (tests/_ard_helpers.ard_grad; for the other two families the same two
expressions with the oracle's Jacobian), fp64 within C_COND cond(Kxx) eps scale / 2, fp32 at F32_GRAD.  The leave-one-out
gradient as tests/test_gpu_loograd.py::test_dloo_against_the_closed_form checks it: tests/_loograd_helpers.loo_grad_reference
(the numpy G), fp64 at ORACLE_TOL, fp32 within C_COND cond eps32 scale with the assertion that the bound does not exceed the
gradient itself.  Data and parameters are that test's (its `_case`) at s = 1."""
import numpy as np
import pytest

import gaussian_processes_amd as gp
from oracle import gp_oracle as orc
from test_gpu_ard import C_COND, F32_GRAD, _nclose, _widths
from test_gpu_loograd import ORACLE_TOL, _check_bound
from _ard_helpers import ard_K, ard_dK, ard_grad, iso_params
from _loograd_helpers import loo_grad_reference, with_noise

pytestmark = pytest.mark.gpu

_EPS = np.finfo(np.float64).eps
S_NOISE = 1.0
SIZES = [1, 63, 64, 65, 129]
FAMILIES = [("gaussian", 3), ("periodic", 1), ("ard", 9)]
_REFS = {}


def _ml_grad(dKs, s, Kinv, alpha):
    """tests/_ard_helpers.ard_grad for any family: (gradient, scale) from the matrices dK/d(kernel parameter)."""
    A = np.outer(alpha, alpha) - Kinv
    aabs, Kabs = np.abs(alpha), np.abs(Kinv)
    grad = [0.5 * float((A * dK).sum()) for dK in dKs]
    scale = [float(aabs @ np.abs(dK) @ aabs) + float((Kabs * np.abs(dK)).sum()) for dK in dKs]
    grad.append(float(s * (alpha @ alpha - np.trace(Kinv))))
    scale.append(2.0 * s * (float(aabs @ aabs) + float(np.abs(np.diag(Kinv)).sum())))
    return np.array(grad), np.array(scale)


def _reference(kind, N, d):
    """x, y, a kernel factory, the marginal-likelihood reference (gradient, scale, cond) and the leave-one-out one
    (value, gradient, G, scale, cond): computed once per (family, N) on the host, shared by both dtypes, never modified."""
    key = (kind, N)
    if key not in _REFS:
        s = S_NOISE
        X, y, _ = orc.synth_inputs(N, d, 1)
        if kind == "ard":
            X = X / 3.0
            h, w = 0.4, _widths(d)
            o = orc.OracleGP("gaussian", iso_params(h, w), X / w, y, s)
            ml = ard_grad(X, h, w, s, o.inv_Kxx, o.inv_Kxx_y)
            K = ard_K(X, X, h, w) + s * s * np.eye(N)
            dKs = with_noise(ard_dK(X, h, w), s)
            make = lambda: gp.GaussianARDKernel(h, w)       # noqa: E731
        else:
            kp = np.array([1.0, 0.5 * np.sqrt(d)]) if kind == "gaussian" else np.array([0.5 * s, 0.8, 3.0])
            o = orc.OracleGP(kind, tuple(kp), X, y, s)
            J = orc.jacobian(kind, X, X, kp)
            ml = _ml_grad(J, s, o.inv_Kxx, o.inv_Kxx_y)
            K = o.Kxx
            dKs = with_noise(J, s)
            cls = gp.GaussianKernel if kind == "gaussian" else gp.PeriodicKernel
            make = lambda: cls(*kp)                         # noqa: E731
        ml = ml + (float(np.linalg.cond(o.Kxx)),)
        loo = loo_grad_reference(K, dKs, y) + (float(np.linalg.cond(K)),)
        _REFS[key] = (X.ravel() if d == 1 else X, y, make, ml, loo)
    return _REFS[key]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind,d", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_both_gradients_on_one_handle_at_the_tile_edges(kind, d, N, dtype):
    x, y, make, (ml_ref, ml_scale, ml_cond), (_, loo_ref, _, loo_scale, loo_cond) = _reference(kind, N, d)
    g = gp.GP(make(), x, y, s=S_NOISE, dtype=dtype)
    what = "%s N=%d d=%d" % (kind, N, d)
    ml, loo = np.array(g.dloglh_dtheta), np.array(g.dloo_dtheta)
    assert ml.shape == ml_ref.shape and loo.shape == loo_ref.shape
    if dtype == "float64":
        for i in range(ml.size):
            _nclose(ml[i], ml_ref[i], C_COND * ml_cond * _EPS, 0.5 * ml_scale[i], "%s dloglh_dtheta[%d]" % (what, i))
        print("%s dloo_dtheta: cond %.2e\n  got %s\n  ref %s" % (what, loo_cond, loo, loo_ref))
        np.testing.assert_allclose(loo, loo_ref, **ORACLE_TOL["float64"])
    else:
        print("%s dloglh_dtheta float32\n  got %s\n  ref %s" % (what, ml, ml_ref))
        np.testing.assert_allclose(ml, ml_ref, **F32_GRAD)
        with np.errstate(invalid="ignore"):     # (periodic, N = 1: d/dp is exactly 0 with bound 0, and the helper prints err / bound)
            _check_bound(loo, loo_ref, loo_scale, loo_cond, dtype, what + " dloo_dtheta")
    # a second call of each, after the other criterion's pass has run on the handle: the same bytes
    del g.dloglh_dtheta, g.dloo_dtheta
    assert np.array(g.dloglh_dtheta).tobytes() == ml.tobytes()
    assert np.array(g.dloo_dtheta).tobytes() == loo.tobytes()
