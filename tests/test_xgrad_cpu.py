"""CPU tests (no GPU needed) of the input-space gradients: the closed forms of tests/_xgrad_helpers.py anchored against
central differences of the oracle's own `mean` / `diag(cov)`, the declarations of the new entries, and what is refused
before the library or a device is touched."""
import os
import re
import subprocess

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib, dist_gp
from oracle import gp_oracle as orc
from conftest import ROOT
from test_dist_gp_cpu import _PythonRBF, no_library      # noqa: F401  (the fixture)
from _xgrad_helpers import RefGP, central_differences

FD_STEP, FD_BOUND = 1e-5, 1e-7      # central differences of step 1e-5: truncation ~ step^2 |f'''| / 6, rounding ~ eps |f| / step

# The finite differences carry the rounding error of the oracle's own cov, about cond(Kxx) eps |k| / step: at step 1e-5 the
# bound needs cond(Kxx) of a few hundred.  The amplitudes keep cond(Kxx) <= 6e2 down to s = 0.1 at both N (asserted below);
# with h = 1 the d = 1 cases reach 6e3 (gaussian) and 4e4 (periodic) and the differences, not the closed forms, miss the bound.
PARAMS = {"gaussian": lambda d: (0.3 if d == 1 else 1.0, 0.5 * np.sqrt(d)), "periodic": lambda d: (0.1 if d == 1 else 0.15, 0.8, 3.0),
          "ard": lambda d: (1.2,) + tuple(np.linspace(0.6, 1.7, d))}
COND_MAX = 6e2
CASES = [("gaussian", 1), ("gaussian", 3), ("gaussian", 8), ("periodic", 1), ("periodic", 2), ("ard", 3)]


@pytest.mark.parametrize("s", [1.0, 0.3, 0.1])
@pytest.mark.parametrize("N", [300, 1100])
@pytest.mark.parametrize("kind,d", CASES, ids=["%s-d%d" % c for c in CASES])
def test_closed_forms_against_central_differences_of_the_oracle(kind, d, N, s):
    X, y, Xo = orc.synth_inputs(N, d, 77)
    ref = RefGP(kind, PARAMS[kind](d), X, y, s)
    lam = np.linalg.eigvalsh(ref.Lxx @ ref.Lxx.T)
    assert lam[-1] / lam[0] <= COND_MAX, lam[-1] / lam[0]
    gm, gv = ref.grads(Xo)
    assert gm.shape == gv.shape == (77, d)
    if kind == "ard":                                       # the oracle has no ARD family: the reference alone
        mean, var = ref.mean, ref.var
    else:                                                   # the oracle's own mean / diag(cov)
        mean, var = ref.o.mean, (lambda p: np.diag(ref.o.cov(p)))
        np.testing.assert_allclose(ref.mean(Xo), mean(Xo), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ref.var(Xo), var(Xo), rtol=1e-9, atol=1e-10)
    for name, got, f in (("mean", gm, mean), ("var", gv, var)):
        fd = central_differences(f, Xo, FD_STEP)
        err, bound = float(np.abs(got - fd).max()), FD_BOUND * max(1.0, float(np.abs(got).max()))
        print("d%s/dx %s d=%d N=%d s=%g: max|analytic| %.3e, |analytic - fd| %.3e, bound %.3e"
              % (name, kind, d, N, s, np.abs(got).max(), err, bound))
        assert err <= bound, (name, err, bound)


PROTOTYPES = [
    "int gpx_d_trsm_right_l(int dtype, const void *L, int64_t n, int64_t ldl, void *X,\n"
    "                       int64_t m, int64_t ldx, void *stream);",
    "int gpx_d_pred_grad(int dtype, int kernel, const void *xo, int64_t m, const void *x, int64_t n, int d,\n"
    "                    const double *params, const void *alpha, const void *B, int64_t ldb, double scale,\n"
    "                    double *out_dev, void *stream);",
    "int gpx_gp_mean_grad(gpx_gp_t *gp, const double *xo, int64_t m, double *grad);",
    "int gpx_gp_var_grad(gpx_gp_t *gp, const double *xo, int64_t m, int64_t chunk_rows, double *var, double *grad);",
]
NAMES = ["gpx_d_trsm_right_l", "gpx_d_pred_grad", "gpx_gp_mean_grad", "gpx_gp_var_grad"]


def test_the_new_entries_are_declared_built_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gpx.h")).read()
    for proto in PROTOTYPES:
        assert proto in hdr, proto
    assert re.search(r"#define GPX_ROUTE_LOO_CHUNK\s+16\b", hdr)
    assert re.search(r"#define GPX_ROUTE_TRSM_L_OPS\s+17\b", hdr)
    assert re.search(r"#define GPX_ROUTE_GRAD_CHUNK\s+18\b", hdr)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert (_lib.ROUTE_LOO_CHUNK, _lib.ROUTE_TRSM_L_OPS, _lib.ROUTE_GRAD_CHUNK) == (16, 17, 18)
    for name in ("dmean_dx", "dvar_dx", "predict_grad"):
        assert callable(getattr(gp.GP, name))
        assert getattr(dist_gp.DistributedGP, name) is not getattr(gp.GP, name)   # refused, not the single-GPU path inherited


def test_refusals_before_the_library_is_touched(no_library):
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    single = gp.GP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1)
    plugin = gp.GP(_PythonRBF(1, 1), x, np.sin(x), s=1)
    dist = gp.DistributedGP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1)
    calls = [lambda g, xo, **kw: g.dmean_dx(xo), lambda g, xo, **kw: g.dvar_dx(xo, **kw), lambda g, xo, **kw: g.predict_grad(xo, **kw)]
    for g in (single, plugin):
        for call in calls:
            with pytest.raises(ValueError, match="invalid shape for xo"):
                call(g, np.zeros((3, 2)))                     # d = 1 here
            with pytest.raises(ValueError, match="invalid shape for xo"):
                call(g, np.zeros((2, 2, 2)))
        for call in calls[1:]:
            with pytest.raises(ValueError, match="chunk_rows"):
                call(g, np.zeros(3), chunk_rows=100)
            with pytest.raises(ValueError, match="chunk_rows"):
                call(g, np.zeros(3), chunk_rows=-128)
    for call in calls:
        with pytest.raises(NotImplementedError, match="plugin contract"):
            call(plugin, np.zeros(3))
        with pytest.raises(NotImplementedError, match="DistributedGP"):
            call(dist, np.zeros(3))


def test_null_and_bad_arguments_are_refused_without_a_device():
    lib = _lib.load()
    out = np.zeros(4)
    assert lib.gpx_gp_mean_grad(None, _lib.dptr(out), 4, _lib.dptr(out)) == _lib.ERR_ARG
    assert lib.gpx_gp_var_grad(None, _lib.dptr(out), 4, 0, None, _lib.dptr(out)) == _lib.ERR_ARG
