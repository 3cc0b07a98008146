"""CPU tests (no GPU needed) of leave-one-out cross-validation: the declarations of the three new entries, the numpy
closed form the GPU tests compare against (checked here by deleting every point in turn on the oracle), and what is
refused before the library or a device is touched."""
import os
import re
import subprocess

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from oracle import gp_oracle as orc
from conftest import ROOT
from test_dist_gp_cpu import no_library      # noqa: F401  (the fixture)
from _loo_helpers import loo_reference

PROTOTYPES = [
    "int gpx_gp_inv_diag(gpx_gp_t *gp, int64_t chunk_rows, double *out);",
    "int gpx_gp_loo(gpx_gp_t *gp, int64_t chunk_rows, double *mean, double *var, double *log_p, double *log_p_sum);",
    "int gpx_d_loo_rows(int dtype, const void *X, int64_t rows, int64_t n, int64_t ldx, int64_t c0, const void *y, const void *alpha,\n"
    "                   double *kii_dev, double *mean_dev, double *var_dev, double *logp_dev, void *stream);",
]
NAMES = ["gpx_gp_inv_diag", "gpx_gp_loo", "gpx_d_loo_rows"]
MEMBERS = ["inv_Kxx_diag", "loo_mean", "loo_var", "loo_log_lh"]


def test_the_three_entries_are_declared_built_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gpx.h")).read()
    for proto in PROTOTYPES:
        assert proto in hdr, proto
    assert re.search(r"#define GPX_ROUTE_LOO_CHUNK\s+16\b", hdr)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert _lib.ROUTE_LOO_CHUNK == 16
    for member in MEMBERS:
        assert isinstance(getattr(gp.GP, member), property)
    assert callable(gp.GP.loo)


@pytest.mark.parametrize("s", [1.0, 0.1])
@pytest.mark.parametrize("kind", ["gaussian", "periodic"])
def test_closed_form_equals_deleting_every_point_in_turn(kind, s):
    n = 40
    d = 3 if kind == "gaussian" else 1
    X, y, _ = orc.synth_inputs(n, d, 1)
    kp = (1.0, 0.5 * np.sqrt(d)) if kind == "gaussian" else (1.0, 0.8, 3.0)
    kii, mean, var, log_p = loo_reference(orc.OracleGP(kind, kp, X, y, s).Kxx, y)
    bmean, bvar = np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        o = orc.OracleGP(kind, kp, X[keep], y[keep], s)
        bmean[i] = o.mean(X[i:i + 1])[0]
        bvar[i] = o.cov(X[i:i + 1])[0, 0] + s * s
    blog_p = -0.5 * np.log(2 * np.pi * bvar) - 0.5 * (y - bmean) ** 2 / bvar
    for name, got, ref in (("mean", mean, bmean), ("var", var, bvar), ("log_p", log_p, blog_p), ("kii", kii, 1.0 / bvar)):
        print("%s s=%g %s: largest difference %.3e" % (kind, s, name, np.abs(got - ref).max()))
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-11, err_msg=name)


def test_bad_chunk_rows_refused_before_the_library(no_library):
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    g = gp.GP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1)
    for bad in (-128, 100):
        with pytest.raises(ValueError, match=r"invalid value for chunk_rows: %d \(0, or a multiple of 128\)" % bad):
            g.loo(chunk_rows=bad)
    assert g._memoized == {}


def test_distributed_gp_points_to_the_single_gpu_class(no_library):
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    g = gp.DistributedGP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1)
    for member in MEMBERS:
        with pytest.raises(NotImplementedError, match="use gp.GP"):
            getattr(g, member)
    with pytest.raises(NotImplementedError, match="use gp.GP"):
        g.loo()
    with pytest.raises(NotImplementedError, match="use gp.GP"):
        g.loo(chunk_rows=128)


def test_null_and_out_of_range_arguments_are_refused_without_a_device():
    lib = _lib.load()
    out = np.zeros(4)
    assert lib.gpx_gp_inv_diag(None, 0, _lib.dptr(out)) == _lib.ERR_ARG
    assert lib.gpx_gp_loo(None, 0, None, None, None, None) == _lib.ERR_ARG
    # a bad dtype, rows < 0, ldx < n, rows that leave the matrix, no input: all before a device is looked for
    assert lib.gpx_d_loo_rows(5, None, 4, 8, 16, 0, None, None, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.gpx_d_loo_rows(_lib.F64, None, -1, 8, 16, 0, None, None, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.gpx_d_loo_rows(_lib.F64, None, 4, 32, 16, 0, None, None, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.gpx_d_loo_rows(_lib.F64, None, 4, 8, 16, 5, None, None, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.gpx_d_loo_rows(_lib.F64, None, 4, 8, 16, 0, None, None, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.gpx_d_loo_rows(_lib.F64, None, 0, 8, 16, 0, None, None, None, None, None, None, None) == _lib.OK
