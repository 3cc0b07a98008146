"""CPU tests (no GPU needed) of the gradient of the leave-one-out criterion: the two numpy forms the GPU tests compare
against (the G form the device runs and RW06 eq. 5.13 as printed) against each other and against central differences of
the numpy criterion, the declarations of the three new entries, and what is decided before the library or a device is
touched (the criterion argument of mlii.optimize, DistributedGP)."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib, mlii
from oracle import gp_oracle as orc
from conftest import ROOT
from test_dist_gp_cpu import no_library      # noqa: F401  (the fixture)
from _loograd_helpers import loo_grad_reference, loo_grad_rw513, loo_value, with_noise

PROTOTYPES = [
    "int gpx_gp_loo_grad(gpx_gp_t *gp, double *loo_log_lh, double *grad);",
    "int gpx_gp_loo_grad_weights(gpx_gp_t *gp, double *G, int64_t ld);",
    "int gpx_gp_fit_batch_loo(gpx_gp_t *gp, const double *thetas, int64_t B, double *loo_log_lh, double *dloo, int *info);",
]
NAMES = ["gpx_gp_loo_grad", "gpx_gp_loo_grad_weights", "gpx_gp_fit_batch_loo"]


def _problem(kind, s, n=40):
    d = 3 if kind == "gaussian" else 1
    X, y, _ = orc.synth_inputs(n, d, 1)
    kp = np.array([1.0, 0.5 * np.sqrt(d)]) if kind == "gaussian" else np.array([1.0, 0.8, 3.0])
    return X, y, kp


def _K(kind, X, kp, s):
    return orc.OracleGP(kind, tuple(kp), X, np.zeros(len(X)), s).Kxx


@pytest.mark.parametrize("s", [1.0, 0.1])
@pytest.mark.parametrize("kind", ["gaussian", "periodic"])
def test_the_two_numpy_forms_agree_and_match_central_differences(kind, s):
    X, y, kp = _problem(kind, s)
    K = _K(kind, X, kp, s)
    J = orc.jacobian(kind, X, X, kp)
    value, grad, G, scale = loo_grad_reference(K, with_noise(J, s), y)
    direct = loo_grad_rw513(K, with_noise(J, s), y)
    print("%s s=%g: G form %s\n  eq. 5.13 %s\n  largest relative difference %.3e" % (kind, s, grad, direct, (np.abs(grad - direct) / np.abs(direct)).max()))
    np.testing.assert_allclose(grad, direct, rtol=1e-12, atol=0)
    assert value == loo_value(K, y)
    # (numpy's inverse is symmetric only to rounding, and so is the G made from it)
    assert np.abs(G - G.T).max() <= 1e-12 * np.abs(G).max() and (scale >= np.abs(grad)).all()
    # central differences with a relative step 1e-6: truncation ~ step^2, rounding ~ eps |L| / step ~ 1e-8 absolute
    theta = np.concatenate([kp, [s]])
    fd = np.empty(theta.size)
    for i in range(theta.size):
        v = []
        for sgn in (-1.0, 1.0):
            t = theta.copy()
            t[i] *= 1.0 + sgn * 1e-6
            v.append(loo_value(_K(kind, X, t[:-1], t[-1]), y))
        fd[i] = (v[1] - v[0]) / (2e-6 * theta[i])
    print("  central differences %s" % fd)
    for g in (grad, direct):
        np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-6 * np.abs(fd).max())


def test_the_three_entries_are_declared_built_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gpx.h")).read()
    for proto in PROTOTYPES:
        assert proto in hdr, proto
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert isinstance(gp.GP.dloo_dtheta, property)
    assert callable(mlii.BatchEvaluator.loo)


def test_a_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    out, th = np.zeros(4), np.ones((1, 3))
    assert lib.gpx_gp_loo_grad(None, _lib.dptr(out), _lib.dptr(out)) == _lib.ERR_ARG
    assert lib.gpx_gp_loo_grad_weights(None, _lib.dptr(out), 2) == _lib.ERR_ARG
    assert lib.gpx_gp_fit_batch_loo(None, _lib.dptr(th), 1, _lib.dptr(out), _lib.dptr(out), None) == _lib.ERR_ARG


def test_optimize_hands_the_criterion_to_the_evaluator_and_maximises_it(no_library):
    centre = np.array([1.3, 2.0, 0.7])

    class Fake(object):
        def __init__(self):
            self.seen, self.threads = [], set()

        def value_and_grad(self, thetas, clamp=True, criterion="log_lh"):
            t = np.atleast_2d(thetas)
            self.seen.append(criterion)
            self.threads.add(threading.get_ident())
            u = np.log(t) - np.log(centre)
            return -(u ** 2).sum(1) * 4.5, -2.0 * u / t * 4.5          # concave in log(theta), maximum 0 at `centre`

    th0 = np.exp(np.random.RandomState(3).uniform(-1.5, 1.5, (5, 3)))
    ev = Fake()
    res = mlii.optimize(None, None, th0, evaluator=ev, maxiter=40, criterion="loo")
    assert set(ev.seen) == {"loo"} and len(ev.seen) == res["batched_calls"] and ev.threads == {threading.get_ident()}
    assert res["criterion"] == "loo"
    assert (res["log_lh"] >= res["log_lh0"]).all()
    np.testing.assert_allclose(res["theta"], np.tile(centre, (5, 1)), rtol=1e-4)
    np.testing.assert_allclose(res["log_lh"], 0.0, atol=1e-7)
    # the default is the marginal likelihood, and an evaluator that has never heard of criteria still serves it
    ev = Fake()
    res = mlii.optimize(None, None, th0, evaluator=ev, maxiter=5)
    assert set(ev.seen) == {"log_lh"} and res["criterion"] == "log_lh"


def test_a_bad_criterion_is_refused_before_the_library(no_library):
    x = np.linspace(0.0, 1.0, 8)
    for bad in ("LOO", "cv", None):
        with pytest.raises(ValueError, match="invalid value for criterion"):
            mlii.optimize(x, np.sin(x), np.ones((2, 3)), criterion=bad)
    ev = mlii.BatchEvaluator.__new__(mlii.BatchEvaluator)             # (no handle: the argument is checked first)
    ev.h = None
    with pytest.raises(ValueError, match="invalid value for criterion"):
        ev.value_and_grad(np.ones((1, 3)), criterion="cv")


def test_distributed_gp_points_to_the_single_gpu_class(no_library):
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    g = gp.DistributedGP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1)
    with pytest.raises(NotImplementedError, match="use gp.GP"):
        g.dloo_dtheta
