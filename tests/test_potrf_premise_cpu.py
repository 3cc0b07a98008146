"""The premise of tests/test_gpu_potrf.py, on the CPU: for every matrix family and size it uses, LAPACK's Cholesky in dtype T
stays below a quarter of the bound the device is held to,

    |A - L L^T|_ij <= 16 K_ij eps_T (|L||L|^T)_ij,    K_ij = min(i, j) + 1 (+ kpre),

so the bound is reachable and a device ratio near 1 is the device's own.  Measured: 0.02 - 0.11 in both dtypes (each case
prints its figure).  Also: the matrices' product L0 L0^T, taken in float64 BLAS on entries that are multiples of 2^-19, IS
the np.longdouble product bit for bit (tests/_block_helpers.py: chol_l0)."""
import numpy as np
import pytest
import scipy.linalg

from _block_helpers import DTYPES, LD, WorstResidual, chol_l0, chol_panel_input, chol_spd

BOTH = pytest.mark.parametrize("dtype", ["f64", "f32"])
PREMISE = 0.25


def test_grid_product_is_the_longdouble_product():
    for n, seed in ((257, 3), (64, 1)):
        l0 = chol_l0(n, seed)
        ld = l0.astype(LD) @ l0.astype(LD).T
        a = chol_spd(n, seed)
        assert np.array_equal(a.astype(LD), ld)
        assert np.array_equal(chol_spd(n, seed, 100).astype(LD), ld[:, :100])
        d = np.diag(l0)
        assert d.min() >= 1.0 and d.max() <= 2.0 and np.array_equal(l0, np.tril(l0))
    assert 5.0 < np.linalg.cond(chol_spd(257, 3)) < 60.0


@BOTH
@pytest.mark.parametrize("n", [64, 257, 700, 1104, 2341])
def test_lapack_factor_is_well_inside_the_bound(dtype, n):
    _, npdt, _, u = DTYPES[dtype]
    a = chol_spd(n, n).astype(npdt)
    l = scipy.linalg.cholesky(a, lower=True)
    assert l.dtype == npdt
    w = WorstResidual("lapack potrf n = %d" % n, dtype)
    w.factor(a, l, u, "n = %d" % n, exact=n <= 700)
    w.report()
    assert w.ratio <= PREMISE


@BOTH
@pytest.mark.parametrize("kpre", [0, 64])
def test_lapack_panel_is_well_inside_the_bound(dtype, kpre):
    """The panel family: the Schur complement behind r0 = 192 columns (kpre of them left to the call), kb = 128 of its columns."""
    _, npdt, _, u = DTYPES[dtype]
    n, r0, kb = 192 + 128 + 65, 192, 128
    s, pre = chol_panel_input(n, 11, r0, n - r0, kpre)
    s, pre = s.astype(npdt), pre.astype(npdt)
    # LAPACK in T on what the device call would see after its own pre-update (taken here in longdouble, rounded once)
    inner = (s.astype(LD) - pre.astype(LD) @ pre.astype(LD).T).astype(npdt)
    l = scipy.linalg.cholesky(inner, lower=True)
    assert l.dtype == npdt
    w = WorstResidual("lapack panel kpre = %d" % kpre, dtype)
    w.factor(s[:, :kb], l[:, :kb], u, "r0 = 192 kb = 128 kpre = %d" % kpre, pre=pre)
    w.report()
    assert w.ratio <= PREMISE
