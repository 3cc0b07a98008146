"""CPU tests of GP.sample_paths (no GPU): the header and the binding of the new entry points, the refusals that come before
the library is touched, and the numpy restatement of the definition (tests/_paths_helpers.py) itself -- its prior is the
kernel, and it conditions on the data."""
import copy
import os
import pickle
import re
from ctypes import POINTER, c_double, c_float, c_int, c_int64, c_uint64, c_void_p

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from conftest import ROOT
from test_dist_gp_cpu import _PythonRBF
from _paths_helpers import cond_bound, kernel_ref, omega_ref, paths_ref, prior_var, view

c_double_p, c_int_p = POINTER(c_double), POINTER(c_int)


# ---- 1. header and bindings ----
def test_paths_symbols_are_declared_and_bound():
    want = {
        "gpx_d_rff_features": (c_int, [c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_double, c_void_p, c_int64, c_void_p]),
        "gpx_d_kmat_apply": (c_int, [c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_double_p, c_void_p, c_int64,
                                     c_int64, c_void_p, c_int64, c_void_p]),
        "gpx_gp_paths_create": (c_int, [c_void_p, c_int64, c_int64, c_uint64, POINTER(c_void_p)]),
        "gpx_paths_eval": (c_int, [c_void_p, c_double_p, c_int64, c_int64, c_double_p]),
        "gpx_paths_get": (c_int, [c_void_p, c_double_p, c_double_p, c_double_p]),
        "gpx_paths_describe": (c_int, [c_void_p, c_int_p, c_int_p, POINTER(c_int64), c_int_p, POINTER(c_int64), POINTER(c_int64),
                                       POINTER(c_uint64)]),
        "gpx_debug_paths_timing": (c_int, [c_void_p, POINTER(c_float)]),
        "gpx_paths_destroy": (c_int, [c_void_p]),
        "gpx_debug_kapply_fused_max": (c_int, [c_int64, POINTER(c_int64)]),
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
    for macro, value in (("GPX_ROUTE_KAPPLY_FUSED", 21), ("GPX_ROUTE_KAPPLY_GEMM", 22), ("GPX_PROF_RFF", 15), ("GPX_PROF_KAPPLY", 16)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr), macro
    assert (_lib.ROUTE_KAPPLY_FUSED, _lib.ROUTE_KAPPLY_GEMM) == (21, 22)
    assert (_lib.PROF_RFF, _lib.PROF_KAPPLY) == (15, 16)
    assert gp.PosteriorPaths is gp.paths.PosteriorPaths and "PosteriorPaths" in gp.__all__


def test_the_route_switch_is_documented_and_works_without_a_gpu():
    """GPX_KAPPLY_FUSED_MAX: a default per dtype in csrc/gpx_tune.h, a section in DESIGN.md, and a process-wide setter that returns the
    value that was in force."""
    tune = open(os.path.join(ROOT, "gaussian_processes_amd", "csrc", "gpx_tune.h")).read()
    for dt in ("F64", "F32"):
        assert int(re.search(r"constexpr int64_t GPX_KAPPLY_FUSED_MAX_%s = (\d+);" % dt, tune).group(1)) >= 1
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "`GPX_KAPPLY_FUSED_MAX`" in design and "Posterior paths" in design
    assert _lib.kapply_fused_max(3) == -1                             # -1: the per-dtype defaults were in force
    assert _lib.kapply_fused_max(0) == 3
    assert _lib.kapply_fused_max(-1) == 0
    assert _lib.kapply_fused_max(-1) == -1


# ---- 2. refusals before the library ----
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def _gp3(K=None):
    rng = np.random.RandomState(0)
    return gp.GP(K or gp.GaussianKernel(1.0, 1.0), rng.randn(10, 3), rng.randn(10), s=1.0)


@pytest.mark.parametrize("kwargs", [
    dict(size=-1), dict(size=2.0), dict(size=(2, 3)), dict(size=True), dict(size=None),
    dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(seed=True),
    dict(features=0), dict(features=-4), dict(features=8.0), dict(features=True), dict(features=None),
], ids=["size_negative", "size_float", "size_tuple", "size_bool", "size_none", "seed_negative", "seed_2_64", "seed_float", "seed_bool",
        "features_zero", "features_negative", "features_float", "features_bool", "features_none"])
def test_sample_paths_refusals_before_the_library(no_library, kwargs):
    args = dict(size=2, seed=1, features=8)
    args.update(kwargs)
    with pytest.raises(ValueError, match=next(iter(kwargs))):
        _gp3().sample_paths(**args)


def test_sample_paths_refuses_other_kernels_before_the_library(no_library):
    x = np.linspace(0, 1, 10)
    for K in (gp.PeriodicKernel(1.0, 1.0, 1.0), _PythonRBF(1.3, 0.9)):
        with pytest.raises(NotImplementedError, match="GaussianKernel and GaussianARDKernel"):
            gp.GP(K, x, np.zeros(10), s=1.0).sample_paths(2, seed=1)
    with pytest.raises(ValueError, match="size"):                     # a bad argument is refused first, whatever the kernel
        gp.GP(gp.PeriodicKernel(1.0, 1.0, 1.0), x, np.zeros(10), s=1.0).sample_paths(-2, seed=1)


def _paths(d, ndim, size=2):
    """A PosteriorPaths object with no device state behind it (the handle is a non-null dummy that is never passed on)."""
    p = gp.PosteriorPaths.__new__(gp.PosteriorPaths)
    p._handle, p.size, p.features, p.seed, p.n, p.d, p._ndim = None, size, 8, 5, 10, d, ndim
    return p


@pytest.mark.parametrize("d,ndim,xo,chunk_rows,what", [
    (3, 2, np.zeros((2, 4)), 0, "xo"), (3, 2, np.zeros(2), 0, "xo"), (3, 2, np.zeros((2, 3, 1)), 0, "xo"), (1, 1, np.zeros((2, 2)), 0, "xo"),
    (1, 2, np.zeros(4), 0, "xo"),
    (3, 2, np.zeros((2, 3)), -128, "chunk_rows"), (3, 2, np.zeros((2, 3)), 100, "chunk_rows"), (3, 2, np.zeros((2, 3)), 128.0, "chunk_rows"),
    (3, 2, np.zeros((2, 3)), True, "chunk_rows"),
], ids=["wrong_d", "xo_1d", "xo_3d", "xo_2d_for_1d", "xo_1d_for_n_by_1", "chunk_negative", "chunk_100", "chunk_float", "chunk_bool"])
def test_paths_call_refusals_before_the_library(no_library, d, ndim, xo, chunk_rows, what):
    with pytest.raises(ValueError, match=what):
        _paths(d, ndim)(xo, chunk_rows=chunk_rows)


def test_paths_are_not_copied_or_pickled(no_library):
    p = _paths(3, 2)
    for f in (copy.copy, copy.deepcopy, pickle.dumps):
        with pytest.raises(NotImplementedError, match=r"regenerate it from the seed.*seed=5"):
            f(p)
    assert (p.size, p.features, p.seed, p.n, p.d) == (2, 8, 5, 10, 3)
    p.close()                                                         # nothing to release: no library needed


def test_distributed_gp_refuses_sample_paths(no_library):
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    dist = gp.DistributedGP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1)
    assert gp.DistributedGP.sample_paths is not gp.GP.sample_paths
    with pytest.raises(NotImplementedError):
        dist.sample_paths(2, seed=1)
    assert "`sample_paths`" in gp.dist_gp.__doc__


# ---- 3. the restatement's prior is the kernel ----
def _pairs(d, widths, rng):
    """4096 point pairs in [-10, 10]^d, half of them within a few widths of each other."""
    a = rng.uniform(-10, 10, (4096, d))
    b = rng.uniform(-10, 10, (4096, d))
    b[:2048] = np.clip(a[:2048] + rng.uniform(-3, 3, (2048, d)) * np.asarray(widths), -10, 10)
    return a, b


@pytest.mark.parametrize("seed", [7, 12345])
@pytest.mark.parametrize("kind,d", [("iso", 1), ("iso", 3), ("ard", 1), ("ard", 3)])
def test_restated_prior_is_the_kernel(kind, d, seed):
    """max over the pairs of |k0 / F sum_f cos(omega_f . (a - b)) - k(a, b)| <= 6 k0 / sqrt(2 F): the feature product
    phi(a) . phi(b) is a mean of F terms k0 cos(omega . (a - b)), each of variance at most k0^2 / 2, around k(a, b); 6
    standard deviations of the worst pair (the restatement gives at most 4.3 over these seeds).  Deterministic."""
    F = 1024
    widths = (0.7, 1.3, 2.9)[:d] if kind == "ard" else (0.8,) * d
    K = gp.GaussianARDKernel(1.3, list(widths)) if kind == "ard" else gp.GaussianKernel(1.3, 0.8)
    a, b = _pairs(d, widths, np.random.RandomState(100 + d))
    pa, h_v, w_v = view(K, a if d > 1 or kind == "ard" else a.ravel())
    pb = view(K, b if d > 1 or kind == "ard" else b.ravel())[0]
    k0 = prior_var(h_v, w_v)
    omega = omega_ref(seed, F, d, w_v)
    approx = k0 / F * np.cos((pa - pb) @ omega.T).sum(axis=1)
    exact = k0 * np.exp(-0.5 * ((pa - pb) ** 2).sum(axis=1) / w_v ** 2)
    unit = k0 / np.sqrt(2.0 * F)
    err = float(np.abs(approx - exact).max())
    print("%s d=%d seed=%d: max err %.3f units of k0 / sqrt(2F)" % (kind, d, seed, err / unit))
    assert np.abs(exact[:64] - np.diag(kernel_ref(pa[:64], pb[:64], h_v, w_v))).max() <= 1e-15 * k0
    assert err <= 6.0 * unit


# ---- 4. the restatement conditions on the data ----
def test_restated_paths_interpolate_noise_free_data():
    """n = 40, d = 1, s = 0, well-spaced x: every path passes through the data, f_s(x_i) = y_i, within the project's
    C_COND cond(Kxx) eps scale."""
    n, S, F, seed = 40, 5, 64, 99
    x = np.linspace(-8, 8, n)
    g = gp.GP(gp.GaussianKernel(1.2, 0.5), x, np.sin(x) + 0.3 * np.cos(3 * x), s=0)
    V, f, info = paths_ref(g, S, F, seed, xo=x)
    bound = cond_bound(info, "float64", "f")
    err = float(np.abs(f - g.y).max())
    print("interpolation: err %.3e bound %.3e cond %.3e" % (err, bound, info["cond"]))
    assert V.shape == (S, n) and f.shape == (S, n)
    assert err <= bound
    assert float(np.abs(f[0] - f[1]).max()) <= 2 * bound                 # ... and so do they all
    off = paths_ref(g, S, F, seed, xo=x[:-1] + 0.2)[1]
    assert float(np.abs(off[0] - off[1]).max()) > 1e-3                   # between the data the paths differ
