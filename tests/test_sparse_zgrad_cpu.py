"""CPU tests of SparseGP's gradient in the inducing inputs: the closed form of tests/_sparse_zgrad_helpers.py against central
differences of the bound of tests/_sparse_helpers.py (the step and tolerance of tests/test_sparse_grad_cpu.py), the conditions
the GPU test's inputs are chosen for, the binding of the new symbols and the refusals that never reach the library."""
from ctypes import POINTER, c_double, c_float, c_int, c_int64, c_size_t, c_void_p
import re

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from conftest import ROOT
from test_gpu_var import C_COND, ORACLE_TOL
from _sparse_helpers import S_NOISE, sgpr_reference
from _sparse_zgrad_helpers import (KEYS, KEY_IDS, key_jitter, make_kernel, median_kernel_ratio, problem, rho32, sgpr_zgrad_reference,
                                   zgrad_reference)

_EPS = float(np.finfo(np.float64).eps)
FD_KEYS = [("gaussian", 129, 3, 65), ("periodic", 129, 1, 65), ("ard", 129, 3, 65)]


@pytest.mark.parametrize("key", FD_KEYS, ids=["%s-%d-%d-%d" % k for k in FD_KEYS])
def test_closed_form_against_central_differences(key):
    kind = key[0]
    params, x, y, z = problem(key)
    jitter = key_jitter(key, "float64")                   # held fixed: it is not differentiated
    closed, scale = sgpr_zgrad_reference(kind, params, x, y, z, S_NOISE, jitter, np.float64)
    assert closed.shape == scale.shape == z.shape and np.isfinite(closed).all() and (scale > 0).all()

    def bound(zz):
        return float(sgpr_reference(kind, params, x, y, zz, S_NOISE, jitter, np.float64)["elbo"])

    worst = 0.0
    flat = closed.ravel()
    for e in range(0, z.size, max(1, z.size // 24)):      # two dozen components spread over the points and dimensions
        step = 1e-5 * max(1.0, abs(z.ravel()[e]))
        up, dn = np.array(z).ravel(), np.array(z).ravel()
        up[e] += step
        dn[e] -= step
        fd = (bound(up.reshape(z.shape)) - bound(dn.reshape(z.shape))) / (2.0 * step)
        ratio = abs(flat[e] - fd) / (1.0 + abs(flat[e]))
        worst = max(worst, ratio)
        print("z[%d]: closed %+.9e  fd %+.9e  |closed - fd| / (1 + |closed|) = %.2e" % (e, flat[e], fd, ratio))
        assert abs(flat[e] - fd) <= 1e-6 * (1.0 + abs(flat[e])), e
    print("%s: largest ratio %.2e" % (key, worst))


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_fp64_references_stand_clear_of_their_tolerance(key):
    """Every component of every fp64 parity key is more than 1e3 times its tolerance: a tolerance that a wrong result could
    hide in would check nothing."""
    ref, scale, cond = zgrad_reference(key)
    tol = np.maximum(ORACLE_TOL["float64"]["atol"] + ORACLE_TOL["float64"]["rtol"] * np.abs(ref), C_COND * cond * _EPS * scale)
    ratio = np.abs(ref) / tol
    print("%s: min |ref| / tol = %.3e  (cond(Kuu) %.2e)" % (key, ratio.min(), cond))
    assert (ratio > 1e3).all(), (key, float(ratio.min()))


@pytest.mark.parametrize("key", [k for k in KEYS if k[0] != "periodic"], ids=[i for k, i in zip(KEYS, KEY_IDS) if k[0] != "periodic"])
def test_the_rectangle_has_entries_that_count(key):
    """median_kernel_ratio's rule: half the entries of K(x, z) are above 1e-5 k(0), so a kernel that mishandled every tile but
    the nearest points' would not pass."""
    med = median_kernel_ratio(key)
    print("%s: median k / k(0) = %.2e" % (key, med))
    assert med > 1e-5, key


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_fp32_floor_does_not_swallow_the_comparison(key):
    """At least 90 % of the components of every fp32 key have a floor below a tenth of the reference."""
    ref, scale, _ = zgrad_reference(key, "float32", np.float64)
    floor = 4.0 * rho32(key) * scale
    share = float(np.mean(floor < 0.1 * np.abs(ref)))
    print("%s: rho = %.3e, floor < 0.1 |ref| for %.1f %% of the components" % (key, rho32(key), 100.0 * share))
    assert share >= 0.9, (key, share)


def test_zgrad_symbols_are_bound():
    want = {
        "gpx_sgp_grad_z": (c_int, [c_void_p, c_int64, POINTER(c_double), POINTER(c_double)]),
        "gpx_sgp_last_zgrad_timing": (c_int, [c_void_p, POINTER(c_float)]),
        "gpx_rect_zgrad_scratch": (c_int, [c_int, c_int64, c_int, POINTER(c_size_t)]),
        "gpx_d_rect_zgrad": (c_int, [c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, POINTER(c_double), c_void_p, c_int64,
                                     c_void_p, c_void_p, c_double, POINTER(c_double), c_void_p, c_void_p, c_void_p]),
    }
    with open(ROOT + "/include/gpx.h") as f:
        hdr = f.read()
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name][0] is res
        assert list(_lib._SIGNATURES[name][1]) == args, name
    assert re.search(r"int gpx_sgp_grad_z\(gpx_sgp_t \*h, int64_t chunk_cols, double \*grad, double \*grad_z\);", hdr)
    assert re.search(r"int gpx_sgp_last_zgrad_timing\(gpx_sgp_t \*h, float \*ms2\);", hdr)
    assert re.search(r"int gpx_d_rect_zgrad\(int dtype, int kernel, const void \*r, int64_t n, const void \*q, int64_t m, int d,", hdr)
    assert _lib.PROF_SPARSE_ZGRAD == 21 and re.search(r"#define GPX_PROF_SPARSE_ZGRAD\s+21\b", hdr)
    assert _lib.PROF_SPARSE_GRAD == 20 and _lib.PROF_SPARSE_GRAM == 19          # the ids that were there keep their numbers
    lib = _lib.load()                                                # (resolves them in the built library)
    assert lib.gpx_sgp_grad_z.argtypes == want["gpx_sgp_grad_z"][1]
    # host arithmetic: enough row slices for (column tiles x windows x slices) to cover the chip at M = 1024, d = 32
    n = c_size_t(0)
    assert lib.gpx_rect_zgrad_scratch(_lib.KERNEL_GAUSSIAN, 1024, 32, n) == 0
    slices = n.value // (1024 * 32)
    assert n.value == slices * 1024 * 32 and (1024 // 64) * slices >= 1024           # (d = 32: one window of dimensions)
    assert lib.gpx_rect_zgrad_scratch(_lib.KERNEL_GAUSSIAN_ARD, 8, 3, n) == _lib.ERR_ARG
    for name in ("delbo_dz", "zgrad_timing"):
        assert hasattr(gp.SparseGP, name)
    assert not hasattr(gp, "delbo_dz")


def test_python_refusals_before_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    key = ("gaussian", 65, 3, 64)
    params, x, y, z = problem(key)
    sg = gp.SparseGP(make_kernel(key[0], params), x, y, S_NOISE, z, jitter=1e-6)
    with pytest.raises(ValueError, match="one \\(lo, hi\\) pair per parameter"):
        sg.optimize(inducing=True, bounds=[(0.1, 10.0)])             # bounds are per PARAMETER: none for z
    with pytest.raises(ValueError, match="one \\(lo, hi\\) pair per parameter"):
        sg.optimize(inducing=True, bounds=[(None, None)] * (3 + z.size))
    for bad in (np.zeros((64, 2)), np.zeros((0, 3)), np.full((64, 3), np.nan)):
        with pytest.raises(ValueError):
            sg.z = bad
    # z has a version of its own: moving it leaves the version of x and y where it is
    xy, zv = sg._xy_version, sg._z_version
    sg.z = z + 1.0
    assert (sg._xy_version, sg._z_version) == (xy, zv + 1) and sg._memoized == {}
    sg.y = y + 1.0
    assert (sg._xy_version, sg._z_version) == (xy + 1, zv + 1)
