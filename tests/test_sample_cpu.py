"""CPU tests of GP.sample: the numpy restatement of the device generator (tests/_sample_helpers.py) against the Random123
known answers and its own structure, the binding of the four new symbols, and the refusals that come before the library is
touched."""
from ctypes import POINTER, c_double, c_int, c_int64, c_uint64, c_void_p

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib
from _sample_helpers import philox4x32_10, randn_ref, z_ref

c_double_p, c_int_p = POINTER(c_double), POINTER(c_int)


# ---- the restatement ----
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    """The Random123 vectors of Philox4x32-10 (kat_vectors: counter, key -> output)."""
    got = " ".join("%08x" % int(w[0]) for w in philox4x32_10(counter, key))
    assert got == want


def test_philox_is_vectorised():
    q = np.array([0, 0xffffffff, 0x243f6a88], dtype=np.uint64)
    out = philox4x32_10((q, [0, 0xffffffff, 0x85a308d3], [0, 0xffffffff, 0x13198a2e], [0, 0xffffffff, 0x03707344]),
                        ([0, 0xffffffff, 0xa4093822], [0, 0xffffffff, 0x299f31d0]))
    assert ["%08x" % int(w) for w in out[0]] == ["6627e8d5", "408f276d", "d16cfe09"]
    assert ["%08x" % int(w) for w in out[3]] == ["9b00dbd8", "6d5451fd", "24126ea1"]


def test_randn_ref_anchor_values():
    got = randn_ref(1, 5, 12345)[0]
    want = [0.28017677, -0.56378626, 2.68381071, -2.13666737, -1.29112166]
    assert np.abs(got - want).max() <= 5e-9              # the 8 digits quoted


def test_randn_ref_structure():
    flat = randn_ref(1, 35, 7)[0]
    assert np.array_equal(randn_ref(5, 7, 7).ravel(), flat)                 # rows x cols with odd cols = the flat sequence
    assert np.array_equal(randn_ref(7, 5, 7).ravel(), flat)
    for off in (1, 2, 13):                                                  # offset shifts the sequence, odd ones too
        assert np.array_equal(randn_ref(1, 35 - off, 7, offset=off)[0], flat[off:])
    assert np.array_equal(randn_ref(2, 7, 7, offset=21).ravel(), flat[21:])
    big = 2 ** 33 + 1
    assert np.array_equal(randn_ref(2, 7, 7, offset=big).ravel(), z_ref(7, 0, np.uint64(big) + np.arange(14, dtype=np.uint64)))
    assert not np.array_equal(randn_ref(1, 35, 7, offset=2 ** 33)[0], flat)          # the high counter word counts
    other = randn_ref(1, 35, 7, stream=1)[0]                                # stream changes it, and so does its high word
    assert not np.any(other == flat)
    assert not np.any(randn_ref(1, 35, 7, stream=2 ** 32)[0] == flat)
    assert not np.any(randn_ref(1, 35, 8)[0] == flat)
    assert not np.any(randn_ref(1, 35, 7 + 2 ** 32)[0] == flat)


@pytest.mark.parametrize("seed", [12345, 0, 2 ** 64 - 1])
def test_randn_ref_moments(seed):
    """N = 2^20: |mean| <= 5 / sqrt(N) = 4.88e-3 and |var - 1| <= 5 sqrt(2 / N) = 6.9e-3 (five standard errors);
    |z| <= sqrt(106 ln 2) = 8.572 by construction (u1 >= 2^-53)."""
    N = 2 ** 20
    z = randn_ref(1, N, seed)[0]
    mean, var = float(z.mean()), float(z.var())
    print("seed %d: mean %.3e var - 1 %.3e max|z| %.3f" % (seed, mean, var - 1.0, float(np.abs(z).max())))
    assert np.all(np.isfinite(z))
    assert abs(mean) <= 5.0 / np.sqrt(N)
    assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / N)
    assert np.abs(z).max() <= 8.572


# ---- bindings ----
def test_sample_symbols_are_bound():
    want = {
        "gpx_d_randn": (c_int, [c_int, c_void_p, c_int64, c_int64, c_int64, c_uint64, c_uint64, c_uint64, c_void_p]),
        "gpx_d_mvn_sample": (c_int, [c_int, c_void_p, c_int64, c_int64, c_void_p, c_double, c_int64, c_uint64, c_uint64, c_void_p,
                                     c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
        "gpx_gp_sample": (c_int, [c_void_p, c_double_p, c_int64, c_int64, c_uint64, c_int, c_double, c_double_p, c_int_p]),
        "gpx_gp_sample_from_K": (c_int, [c_void_p, c_double_p, c_double_p, c_int64, c_int64, c_uint64, c_int, c_double, c_double_p,
                                         c_int_p]),
    }
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert _lib._SIGNATURES[name][0] is res
        assert list(_lib._SIGNATURES[name][1]) == args, name
    assert _lib.ROUTE_SAMPLE == 20
    assert _lib.PROF_RANDN == 14
    lib = _lib.load()
    for name in want:
        assert hasattr(lib, name)


# ---- refusals ----
@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def _gp3():
    rng = np.random.RandomState(0)
    return gp.GP(gp.GaussianKernel(1.0, 1.0), rng.randn(10, 3), rng.randn(10), s=1.0)


@pytest.mark.parametrize("kwargs", [
    dict(xo=np.zeros((2, 4))),                  # wrong d
    dict(xo=np.zeros(2)),                       # (m,) for 3-D inputs
    dict(xo=np.zeros((2, 3, 1))),               # 3-D xo
    dict(size=-1),
    dict(size=2.0),
    dict(size=(2, 3)),
    dict(size=True),
    dict(seed=-1),
    dict(seed=2 ** 64),
    dict(seed=1.5),
    dict(jitter=-1e-9),
    dict(jitter=np.nan),
    dict(jitter=np.inf),
    dict(jitter="big"),
], ids=["wrong_d", "xo_1d", "xo_3d", "size_negative", "size_float", "size_tuple", "size_bool", "seed_negative", "seed_2_64",
        "seed_float", "jitter_negative", "jitter_nan", "jitter_inf", "jitter_str"])
def test_sample_refusals_before_the_library(no_library, kwargs):
    g = _gp3()
    args = dict(xo=np.zeros((2, 3)), seed=1)
    args.update(kwargs)
    with pytest.raises(ValueError):
        g.sample(**args)


def test_sample_refusals_1d(no_library):
    g = gp.GP(gp.GaussianKernel(1.0, 1.0), np.linspace(0, 1, 10), np.zeros(10), s=1.0)
    with pytest.raises(ValueError, match="invalid shape for xo"):
        g.sample(np.zeros((2, 2)), seed=1)
    with pytest.raises(ValueError, match="size"):
        g.sample(np.zeros(2), size=-3)


def test_distributed_gp_refuses_sample(no_library):
    x = np.linspace(-2 * np.pi, 2 * np.pi, 16)
    dist = gp.DistributedGP(gp.GaussianKernel(1, 1), x, np.sin(x), s=1)
    assert gp.DistributedGP.sample is not gp.GP.sample          # refused, not the single-GPU path inherited
    with pytest.raises(NotImplementedError):
        dist.sample(np.zeros(1), seed=1)
    assert "`sample`" in gp.dist_gp.__doc__
