"""CPU tests (no GPU needed) of gp.DistributedGP's host-side contract and of the gpx_mg_cov declaration: what is refused
happens before the library is touched."""
import os
import pickle
import re
from copy import copy, deepcopy

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib, dist_gp, multi_gpu
from conftest import ROOT


class _PythonRBF(gp.kernels.Kernel):
    """A pure-Python kernel plugin (no native id)."""

    def __init__(self, h, ell):
        self.h, self.ell = float(h), float(ell)

    @property
    def params(self):
        return np.array([self.h, self.ell])

    @params.setter
    def params(self, val):
        self.h, self.ell = float(val[0]), float(val[1])

    def K(self, x1, x2, out=None):
        a = np.asarray(x1, dtype=np.float64).reshape(len(x1), -1)
        b = np.asarray(x2, dtype=np.float64).reshape(len(x2), -1)
        return self.h ** 2 * np.exp(-0.5 * ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1) / self.ell ** 2)


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to reach libgpx or to create a distributed handle fails the test."""
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(multi_gpu, "NativeDistributedGP", boom)


def _make(**kw):
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    return gp.DistributedGP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1, **kw)


def test_exported_from_the_package():
    assert gp.DistributedGP is dist_gp.DistributedGP
    assert issubclass(gp.DistributedGP, gp.GP)
    assert "DistributedGP" in gp.__all__


def test_gpx_mg_cov_is_declared_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpx.h")).read(), flags=re.S)
    assert re.search(r"int gpx_mg_cov\(gpx_mg_t \*mg, const double \*params, const double \*xo, int64_t m, double \*out\);", hdr)
    assert "gpx_mg_cov" in _lib.EXPORTED_SYMBOLS
    assert hasattr(multi_gpu.NativeDistributedGP, "cov")
    assert issubclass(multi_gpu.RankMismatchError, _lib.GpxError)


def test_plugin_kernel_refused_before_the_library(no_library):
    x = np.linspace(0, 1, 8)
    with pytest.raises(TypeError, match="built-in kernel"):
        gp.DistributedGP(_PythonRBF(1, 1), x, np.sin(x))


def test_bad_shapes_refused_before_the_library(no_library):
    with pytest.raises(ValueError, match="invalid shape for x"):
        gp.DistributedGP(gp.GaussianKernel(1, 1), np.zeros((2, 2, 2)), np.zeros(2))
    with pytest.raises(ValueError, match="invalid shape for y"):
        gp.DistributedGP(gp.GaussianKernel(1, 1), np.zeros(5), np.zeros(4))
    with pytest.raises(ValueError, match="invalid value for s"):
        gp.DistributedGP(gp.GaussianKernel(1, 1), np.zeros(5), np.zeros(5), s=-1)
    with pytest.raises(ValueError, match="backend"):
        _make(backend="mpi")
    g = _make()
    with pytest.raises(ValueError, match="invalid shape for xo"):
        g.cov(np.zeros((3, 2)))                  # d = 1 here
    with pytest.raises(ValueError, match="invalid shape for xo"):
        g.mean(np.zeros((2, 2, 2)))


def test_copy_and_pickle_raise(no_library):
    g = _make()
    for f in (lambda: copy(g), lambda: deepcopy(g), lambda: g.copy(), lambda: pickle.dumps(g),
              lambda: pickle.dumps(g, protocol=0)):
        with pytest.raises(NotImplementedError, match="use gp.GP"):
            f()


@pytest.mark.parametrize("member", ["Kxx", "Kxx_J", "Kxx_H", "Lxx", "inv_Kxx", "dloglh_dtheta", "dlh_dtheta",
                                    "d2lh_dtheta2", "d2loglh_dtheta2"])
def test_host_matrix_members_point_to_gp(no_library, member):
    g = _make()
    with pytest.raises(NotImplementedError, match="use gp.GP"):
        getattr(g, member)


def test_host_methods_point_to_gp(no_library, tmp_path):
    g = _make()
    with pytest.raises(NotImplementedError, match="use gp.GP"):
        g.dm_dtheta(np.zeros(3))
    with pytest.raises(NotImplementedError, match="use gp.GP"):
        g.save_fitted(str(tmp_path / "f.gpx"))
    with pytest.raises(NotImplementedError, match="use gp.GP"):
        gp.DistributedGP.load_fitted(str(tmp_path / "f.gpx"))


def test_setters_invalidate_like_gp(no_library):
    g = _make()
    g._memoized["log_lh"] = 1.0
    v = g._version
    g.params = np.array([2.0, 1.0, 1.0])
    assert g._memoized == {} and g._version > v
    g._memoized["log_lh"] = 1.0
    g.set_param("w", 3.0)
    assert g._memoized == {} and g.K.w == 3.0
    g._memoized["log_lh"] = 1.0
    g.s = 0.5
    assert g._memoized == {}


def test_a_new_n_or_d_is_a_change(no_library):
    g = _make()
    g._memoized["log_lh"] = 1.0
    v = g._data_version
    g.x, g.y = np.linspace(0, 1, 20), np.zeros(20)
    assert g._memoized == {} and g._data_version > v and g._n == 20
    g.x = np.zeros((20, 3))
    assert (g._n, g._d) == (20, 3)
    with pytest.raises(ValueError, match="invalid shape for y"):
        g.y = np.zeros(21)
