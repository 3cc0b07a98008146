"""CPU tests of PosteriorPaths.grad / value_and_grad (no GPU): the header and the binding of the new entry points, the
refusals that come before the library is touched, and the numpy restatement of a path's gradient
(tests/_paths_grad_helpers.py) itself -- against central differences of `paths_ref`, and at the data of a noise-free fit."""
import os
import re
from ctypes import POINTER, c_double, c_int, c_int64, c_void_p

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from conftest import ROOT
from _paths_helpers import paths_ref
from _paths_grad_helpers import grad_ref

c_double_p = POINTER(c_double)


# ---- 1. header and bindings ----
def test_paths_grad_symbols_are_declared_and_bound():
    want = {
        "gpx_d_rff_features_grad": (c_int, [c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_double, c_double_p, c_void_p,
                                            c_int64, c_void_p]),
        "gpx_d_kmat_apply_grad": (c_int, [c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_double_p, c_double_p, c_void_p,
                                          c_int64, c_int64, c_void_p, c_int64, c_void_p]),
        "gpx_paths_grad": (c_int, [c_void_p, c_double_p, c_int64, c_int64, c_double_p, c_double_p]),
    }
    hdr = open(os.path.join(ROOT, "include", "gpx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name, (res, args) in want.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), "include/gpx.h does not declare %s" % name
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name][0] is res
        assert list(_lib._SIGNATURES[name][1]) == args, name
        assert hasattr(lib, name)
    for macro, value in (("GPX_ROUTE_PATHS_GRAD_CHUNK", 23), ("GPX_PROF_KAPPLY_GRAD", 17)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr), macro
    assert (_lib.ROUTE_PATHS_GRAD_CHUNK, _lib.PROF_KAPPLY_GRAD) == (23, 17)
    assert callable(gp.PosteriorPaths.grad) and callable(gp.PosteriorPaths.value_and_grad)
    for doc in (gp.paths.__doc__, gp.GP.sample_paths.__doc__):
        assert "value_and_grad" in doc and "gradients of a path" not in doc


# ---- 2. refusals before the library ----
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def _paths(d, ndim, size=2):
    """A PosteriorPaths object with no device state behind it (the handle is a dummy that is never passed on)."""
    p = gp.PosteriorPaths.__new__(gp.PosteriorPaths)
    p._handle, p.size, p.features, p.seed, p.n, p.d, p._ndim = None, size, 8, 5, 10, d, ndim
    return p


@pytest.mark.parametrize("method", ["grad", "value_and_grad"])
@pytest.mark.parametrize("d,ndim,xo,chunk_rows,what", [
    (3, 2, np.zeros((2, 4)), 0, "xo"), (3, 2, np.zeros(2), 0, "xo"), (3, 2, np.zeros((2, 3, 1)), 0, "xo"), (1, 1, np.zeros((2, 2)), 0, "xo"),
    (1, 2, np.zeros(4), 0, "xo"),
    (3, 2, np.zeros((2, 3)), -128, "chunk_rows"), (3, 2, np.zeros((2, 3)), 100, "chunk_rows"), (3, 2, np.zeros((2, 3)), 128.0, "chunk_rows"),
    (3, 2, np.zeros((2, 3)), True, "chunk_rows"),
], ids=["wrong_d", "xo_1d", "xo_3d", "xo_2d_for_1d", "xo_1d_for_n_by_1", "chunk_negative", "chunk_100", "chunk_float", "chunk_bool"])
def test_paths_grad_refusals_before_the_library(no_library, method, d, ndim, xo, chunk_rows, what):
    with pytest.raises(ValueError, match=what):
        getattr(_paths(d, ndim), method)(xo, chunk_rows=chunk_rows)


@pytest.mark.parametrize("method", ["grad", "value_and_grad", "__call__"])
def test_closed_paths_refuse_before_the_library(no_library, method):
    with pytest.raises(ValueError, match="closed"):
        getattr(_paths(3, 2), method)(np.zeros((2, 3)))


# ---- 3. the restatement against central differences of paths_ref ----
def _case(kind):
    rng = np.random.RandomState(3)
    if kind == "gauss1":
        x = np.linspace(-8, 8, 40)
        return gp.GP(gp.GaussianKernel(1.2, 0.5), x, np.sin(x) + 0.3 * np.cos(3 * x), s=0.5), rng.uniform(-8, 8, 25)
    x = rng.uniform(-3, 3, (60, 3))
    y = np.sin(x[:, 0]) + 0.3 * np.cos(x[:, 1] - 0.5 * x[:, 2])
    K = gp.GaussianKernel(1.0, 0.5 * np.sqrt(3)) if kind == "gauss3" else gp.GaussianARDKernel(1.0, [0.7, 1.1, 1.6])
    return gp.GP(K, x, y, s=0.5), rng.uniform(-3, 3, (25, 3))


@pytest.mark.parametrize("kind", ["gauss1", "gauss3", "ard3"])
def test_restated_gradient_matches_central_differences(kind):
    """Step 1e-5, tolerance 1e-7 max(1, max|G|) -- the one tests/test_gpu_xgrad.py uses for the same comparison (the
    truncation error h^2 / 6 |f'''| and the rounding error eps |f| / h of a central difference are both below it)."""
    S, F, seed, step = 5, 64, 99, 1e-5
    g, xo = _case(kind)
    f, G, info = grad_ref(g, S, F, seed, xo)
    pts = xo.reshape(len(xo), -1)
    d = pts.shape[1]
    assert f.shape == (S, 25) and G.shape == (S, 25, d) and info["scale_g"] > 0
    num = np.empty_like(G)
    for k in range(d):
        e = np.zeros(d)
        e[k] = step
        up, dn = (pts + e).reshape(xo.shape), (pts - e).reshape(xo.shape)
        num[:, :, k] = (paths_ref(g, S, F, seed, xo=up)[1] - paths_ref(g, S, F, seed, xo=dn)[1]) / (2 * step)
    err, tol = float(np.abs(G - num).max()), 1e-7 * max(1.0, float(np.abs(G).max()))
    print("%s: max|G| %.3f err %.3e tol %.3e ratio %.3e" % (kind, float(np.abs(G).max()), err, tol, err / tol))
    assert err <= tol


# ---- 4. noise-free data: the values interpolate, the slopes do not ----
def test_restated_gradient_at_noise_free_data():
    n, S, F, seed = 40, 5, 64, 99
    x = np.linspace(-8, 8, n)
    g = gp.GP(gp.GaussianKernel(1.2, 0.5), x, np.sin(x) + 0.3 * np.cos(3 * x), s=0)
    f, G, info = grad_ref(g, S, F, seed, x)
    assert G.shape == (S, n, 1) and np.all(np.isfinite(G))
    assert float(np.abs(f[0] - f[1]).max()) < 1e-6                       # every path passes through the data ...
    assert float(np.abs(G[0] - G[1]).max()) > 1e-3                       # ... at a slope of its own
