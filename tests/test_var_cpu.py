"""CPU tests (no GPU needed) of the chunked predictive variance: the declarations of the five new entries, the host
arithmetic of the row chunking (gpx_debug_var_plan), `Kernel.diag`, and what is refused before the library or a device
is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib, dist_gp, multi_gpu
from oracle import gp_oracle as orc
from conftest import ROOT
from test_dist_gp_cpu import _PythonRBF, no_library      # noqa: F401  (the fixture)

PROTOTYPES = [
    "int gpx_d_var_rows(int dtype, int kernel, const void *X, int64_t rows, int64_t n, int64_t ldx, const void *xo, int d,\n"
    "                   const double *params, const double *kdiag_dev, double *out_dev, void *stream);",
    "int gpx_gp_var(gpx_gp_t *gp, const double *xo, int64_t m, int64_t chunk_rows, double *out);",
    "int gpx_gp_var_from_K(gpx_gp_t *gp, const double *Kxox, const double *kdiag, int64_t m, int64_t chunk_rows, double *out);",
    "int gpx_debug_var_plan(int dtype, int64_t n, int64_t m, int64_t chunk_rows, size_t free_bytes,\n"
    "                       int64_t *rows_per_chunk, int64_t *chunks, size_t *bytes_per_chunk);",
    "int gpx_mg_var(gpx_mg_t *mg, const double *params, const double *xo, int64_t m, int64_t chunk_rows, double *out);",
]
NAMES = ["gpx_d_var_rows", "gpx_gp_var", "gpx_gp_var_from_K", "gpx_debug_var_plan", "gpx_mg_var"]


def test_the_five_entries_are_declared_built_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gpx.h")).read()
    for proto in PROTOTYPES:
        assert proto in hdr, proto
    assert re.search(r"#define GPX_ROUTE_VAR_CHUNK\s+15\b", hdr)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert _lib.ROUTE_VAR_CHUNK == 15
    for cls in (gp.GP, gp.DistributedGP, dist_gp.DistributedGP):
        assert callable(getattr(cls, "var")) and callable(getattr(cls, "predict"))
    assert callable(multi_gpu.NativeDistributedGP.var)
    assert gp.DistributedGP.var is not gp.GP.var               # the collective form, not the single-GPU one inherited
    assert gp.DistributedGP.predict is not gp.GP.predict


def _plan(dtype, n, m, chunk_rows, free_bytes):
    rows, chunks, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_size_t(0)
    rc = _lib.load().gpx_debug_var_plan(dtype, n, m, chunk_rows, free_bytes, ctypes.byref(rows), ctypes.byref(chunks),
                                        ctypes.byref(nbytes))
    return rc, rows.value, chunks.value, int(nbytes.value)


@pytest.mark.parametrize("dtype", [_lib.F64, _lib.F32])
@pytest.mark.parametrize("n", [1000, 8192, 65536, 131072])
def test_plan_properties(dtype, n):
    es = 8 if dtype == _lib.F64 else 4
    row_bytes = (n + 15) // 16 * 16 * es                      # the chunk buffer alone: a lower bound of a row's cost
    for free in (256 << 30, 32 << 30, 3 << 30, 1 << 30):
        for m in (0, 1, 127, 128, 4097, 10 ** 6):
            rc, rows, chunks, nbytes = _plan(dtype, n, m, 0, free)
            if 128 * row_bytes > free // 4:                   # 128 rows cannot fit: the only admissible answer
                assert rc == _lib.ERR_NOMEM, (n, m, free)
                continue
            assert rc == _lib.OK, (n, m, free, _lib.last_error())
            assert rows % 128 == 0 or (rows == m and chunks == 1), (rows, m)
            assert rows >= 1 and chunks * rows >= m > (chunks - 1) * rows, (rows, chunks, m)
            assert rows * row_bytes <= nbytes <= free // 4, (rows, nbytes, free)
            if m > 0 and chunks > 1:
                assert rows >= 128
            # an explicit chunk size is honoured (when it fits), whatever the automatic figure is
            for want in (128, 1024):
                rc2, rows2, chunks2, nbytes2 = _plan(dtype, n, m, want, free)
                if want * row_bytes > free // 4 and m >= want:
                    assert rc2 == _lib.ERR_NOMEM
                    continue
                if rc2 == _lib.ERR_NOMEM:                     # (between the lower bound and the real per-row cost)
                    continue
                assert rc2 == _lib.OK
                assert rows2 == (want if m == 0 or m > want else m), (rows2, want, m)
                assert chunks2 * rows2 >= m > (chunks2 - 1) * rows2
                assert nbytes2 <= free // 4


def test_plan_numbers_at_the_headline_size():
    """N = 65536 fp64 on an empty 288 GB device: chunks of the 4096-row cap, 16 of them at m = 65536, each well under a
    quarter of the memory; m = 200 000 at N = 8192 is 49 chunks."""
    rc, rows, chunks, nbytes = _plan(_lib.F64, 65536, 65536, 0, 280 << 30)
    assert (rc, rows, chunks) == (_lib.OK, 4096, 16)
    assert 4096 * 65536 * 8 <= nbytes <= 4096 * (65536 + 1024) * 8
    assert _plan(_lib.F64, 8192, 200000, 0, 280 << 30)[1:3] == (4096, 49)
    assert _plan(_lib.F64, 8192, 1000, 128, 280 << 30)[1:3] == (128, 8)
    assert _plan(_lib.F64, 8192, 1000, 0, 280 << 30)[1:3] == (1000, 1)


def test_plan_refusals():
    for bad in (1, 100, 127, 129, 4000, -128):
        assert _plan(_lib.F64, 8192, 1000, bad, 1 << 40)[0] == _lib.ERR_ARG, bad
    assert "multiple of 128" in _lib.last_error()
    assert _plan(_lib.F64, 8192, -1, 0, 1 << 40)[0] == _lib.ERR_ARG
    assert _plan(_lib.F64, 0, 10, 0, 1 << 40)[0] == _lib.ERR_ARG
    assert _plan(7, 8192, 10, 0, 1 << 40)[0] == _lib.ERR_ARG
    # 128 rows of 65536 doubles are 64 MiB: a quarter of 128 MiB does not hold them, of 1 GiB it does
    assert _plan(_lib.F64, 65536, 1000, 0, 128 << 20)[0] == _lib.ERR_NOMEM
    assert _plan(_lib.F64, 65536, 1, 0, 128 << 20)[0] == _lib.ERR_NOMEM
    assert _plan(_lib.F64, 65536, 1000, 0, 1 << 30)[0] == _lib.OK
    assert _plan(_lib.F64, 65536, 5000, 4096, 1 << 30)[0] == _lib.ERR_NOMEM      # an explicit chunk that does not fit
    assert _plan(_lib.F64, 65536, 1000, 0, 0)[0] == _lib.ERR_NOMEM


@pytest.mark.parametrize("d", [1, 3])
def test_closed_form_diag_equals_the_oracles_diagonal(d):
    rng = np.random.RandomState(3)
    X = rng.uniform(-10, 10, (50, d))
    x = X.ravel() if d == 1 else X
    for h, w in [(1.0, 1.0), (0.7, 1.3), (3.1, 0.05)]:
        got = gp.GaussianKernel(h, w).diag(x)
        assert got.shape == (50,) and got.dtype == np.float64
        np.testing.assert_allclose(got, np.diag(orc.kernel_matrix("gaussian", "K", X, X, (h, w))), rtol=1e-15, atol=0)
    for h, w, p in [(1.0, 1.0, 1.0), (0.7, 1.3, 2.0), (2.5, 0.3, 7.0)]:
        got = gp.PeriodicKernel(h, w, p).diag(x)
        assert got.shape == (50,) and got.dtype == np.float64
        np.testing.assert_allclose(got, np.diag(orc.kernel_matrix("periodic", "K", X, X, (h, w, p))), rtol=1e-15, atol=0)
    assert gp.GaussianKernel(1, 1).diag(np.zeros((0, d))).shape == (0,)
    bad = X.copy()
    bad[4, 0] = np.inf
    assert np.isnan(gp.GaussianKernel(1, 1).diag(bad)[4]) and np.isfinite(np.delete(gp.GaussianKernel(1, 1).diag(bad), 4)).all()


def test_plugin_kernel_default_diag():
    k = _PythonRBF(1.3, 0.7)
    for x in (np.linspace(-2, 2, 9), np.random.RandomState(0).randn(9, 3)):
        got = k.diag(x)
        assert got.shape == (9,) and got.dtype == np.float64
        np.testing.assert_array_equal(got, np.diag(k.K(x, x)))
    assert "diag" not in _PythonRBF.__dict__                  # the base class's loop, not an override


def test_bad_xo_and_chunk_rows_refused_before_the_library(no_library):
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    single = gp.GP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1)
    dist = gp.DistributedGP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1)
    plugin = gp.GP(_PythonRBF(1, 1), x, np.sin(x), s=1)
    for g in (single, dist, plugin):
        with pytest.raises(ValueError, match="invalid shape for xo"):
            g.var(np.zeros((3, 2)))                           # d = 1 here
        with pytest.raises(ValueError, match="invalid shape for xo"):
            g.var(np.zeros((2, 2, 2)))
        with pytest.raises(ValueError, match="invalid shape for xo"):
            g.predict(np.zeros((3, 2)))
    for g in (single, plugin):
        with pytest.raises(ValueError, match="chunk_rows"):
            g.var(np.zeros(3), chunk_rows=100)
        with pytest.raises(ValueError, match="chunk_rows"):
            g.var(np.zeros(3), chunk_rows=-128)


def test_null_and_negative_arguments_are_refused_without_a_device():
    lib = _lib.load()
    out = np.zeros(4)
    assert lib.gpx_gp_var(None, _lib.dptr(out), 4, 0, _lib.dptr(out)) == _lib.ERR_ARG
    assert lib.gpx_gp_var(None, None, -1, 0, None) == _lib.ERR_ARG
    assert lib.gpx_gp_var_from_K(None, _lib.dptr(out), _lib.dptr(out), 4, 0, _lib.dptr(out)) == _lib.ERR_ARG
    assert lib.gpx_mg_var(None, _lib.dptr(out), _lib.dptr(out), 4, 0, _lib.dptr(out)) == _lib.ERR_ARG
    p = np.array([1.0, 1.0])
    # rows < 0, ldx < n, a bad dtype, no output, neither kdiag nor (xo, params): all before a device is looked for
    assert lib.gpx_d_var_rows(_lib.F64, _lib.KERNEL_GAUSSIAN, None, -1, 8, 16, None, 1, _lib.dptr(p), None, None, None) == _lib.ERR_ARG
    assert lib.gpx_d_var_rows(_lib.F64, _lib.KERNEL_GAUSSIAN, None, 4, 32, 16, None, 1, _lib.dptr(p), None, None, None) == _lib.ERR_ARG
    assert lib.gpx_d_var_rows(5, _lib.KERNEL_GAUSSIAN, None, 4, 8, 16, None, 1, _lib.dptr(p), None, None, None) == _lib.ERR_ARG
    assert lib.gpx_d_var_rows(_lib.F64, _lib.KERNEL_GAUSSIAN, None, 4, 0, 16, None, 1, _lib.dptr(p), None, None, None) == _lib.ERR_ARG
    assert lib.gpx_d_var_rows(_lib.F64, _lib.KERNEL_GAUSSIAN, None, 0, 8, 16, None, 1, None, None, None, None) == _lib.OK
