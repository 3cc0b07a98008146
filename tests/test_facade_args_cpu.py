"""Characterisation table of the Python facades' host plumbing: one row per argument rule and call site -- the call, and either
the exception type with its FULL message (raised before the library is touched) or the normalised value that reaches the
library -- plus the route every derivative member takes for every kernel family, and the dtype table.

No GPU and no built library: `_lib.load` is patched to a recording stand-in whose entries return GPX_OK and write nothing,
except the entries of `STOPS`, which end the call and hand back their arguments.

The rows marked CHANGED are the one deliberate change of the consolidation into `_facade.py`, the `mlii` dtype fallback; every
other row states what the five facade modules did before it, call site by call site.
"""
import ctypes

import numpy as np
import pytest

import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib, mlii

STOPS = {"gpx_gp_var", "gpx_gp_var_grad", "gpx_gp_loo", "gpx_sgp_var", "gpx_paths_eval", "gpx_paths_grad", "gpx_gp_sample",
         "gpx_gp_paths_create", "gpx_sgp_select", "gpx_gp_dloglh_dtheta", "gpx_gp_get_inv_Kxx", "gpx_gp_loo_grad",
         "gpx_gp_loo_grad_weights", "gpx_gp_dlh_d2lh", "gpx_gp_dm_dtheta", "gpx_gp_mean_grad"}


class Reached(Exception):
    def __init__(self, entry, args):
        Exception.__init__(self, entry)
        self.entry, self.args_seen = entry, args


class RecordingLibrary(object):
    """Stands in for libgpx.so: every ``gpx_*`` entry is recorded and returns GPX_OK; an entry of `stops` raises `Reached`."""

    def __init__(self, stops=STOPS):
        self.stops, self.calls = set(stops), []

    def __getattr__(self, name):
        if not name.startswith("gpx_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            if name in self.stops:
                raise Reached(name, args)
            return _lib.OK
        return entry


@pytest.fixture
def lib(monkeypatch):
    fake = RecordingLibrary()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    return fake


class _Plugin(gp.Kernel):
    """A pure-Python kernel plugin (no native id)."""

    def __init__(self, h, ell):
        self.h, self.ell = float(h), float(ell)

    @property
    def params(self):
        return np.array([self.h, self.ell])

    def K(self, x1, x2, out=None):
        a = np.asarray(x1, dtype=np.float64).reshape(len(x1), -1)
        b = np.asarray(x2, dtype=np.float64).reshape(len(x2), -1)
        return self.h ** 2 * np.exp(-0.5 * ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1) / self.ell ** 2)


KERNELS = {"gaussian": lambda d: gp.GaussianKernel(1.0, 1.0), "periodic": lambda d: gp.PeriodicKernel(1.0, 1.0, 1.0),
           "ard": lambda d: gp.GaussianARDKernel(1.0, [1.0] * d), "plugin": lambda d: _Plugin(1.0, 1.0)}
N = 10
Y = np.arange(float(N))


def _x(d):
    """(N,) for d = 1 -- the reference's 1-D inputs -- and (N, d) otherwise; d = "n1": (N, 1)."""
    rng = np.random.RandomState(0)
    return rng.randn(N, 1) if d == "n1" else rng.randn(N) if d == 1 else rng.randn(N, d)


def _xo(d, m=4):
    return np.zeros(m) if d == 1 else np.zeros((m, d))


def _gp(d=3, kernel="gaussian", **kw):
    return gp.GP(KERNELS[kernel](d), _x(d), Y, s=1.0, **kw)


def _sgp(d=3, K=None, **kw):
    x = _x(d)
    return gp.SparseGP(K or gp.GaussianKernel(1.0, 1.0), x, Y, 1.0, x[:4], **kw)


def _on_paths(method, xo, chunk_rows=0, d=3, ndim=2):
    """`method` of a PosteriorPaths object over a non-null dummy handle, which is taken away again before the object goes."""
    p = gp.PosteriorPaths(ctypes.c_void_p(1), 2, 8, 5, N, d, ndim)
    try:
        return getattr(p, method)(xo, chunk_rows=chunk_rows)
    finally:
        p._handle = None


# ---- what a row expects ----
def raises(exc, message):
    return ("raises", exc, message)


def arg(entry, index, value):
    """The call is accepted and reaches `entry` with `value` (and its type) as argument `index`."""
    return ("arg", entry, index, value)


def returns(value):
    return ("returns", value)


def _check(lib, call, expect):
    del lib.calls[:]
    try:
        got = ("returns", call())
    except Reached as r:
        got = ("reached", r.entry, r.args_seen)
    except Exception as exc:      # noqa: BLE001 -- the row says which
        got = ("raises", type(exc), str(exc))
    if expect[0] == "raises":
        assert got == expect, got[:2] + (got[2] if got[0] == "raises" else "...",)
        assert lib.calls == [], "refused after the library was touched: %s" % [c[0] for c in lib.calls]
    elif expect[0] == "arg":
        _, entry, index, value = expect
        assert got[:2] == ("reached", entry), got[:2] + (str(got[2])[:200],)
        seen = got[2][index]
        assert seen == value and type(seen) is type(value), (seen, value)
    else:
        assert got == expect


ROWS = []


def row(name, call, expect):
    ROWS.append(pytest.param(call, expect, id=name))


# ---- chunk_rows / chunk_cols: the lenient rule (int() first) and the strict one (PosteriorPaths: no bools, no floats) ----
CHUNK_VALUES = (0, 128, 256, -128, 100, 128.0, True, "128")
CHUNK_MSG = "invalid value for %s: %s (0, or a multiple of 128)"
LENIENT = (0, 128, 256, "-128", "100", 128, "1", 128)                     # per value: accepted as (int), or refused and shown as (str)
STRICT = (0, 128, 256, "-128", "100", "128.0", "True", "'128'")


def _chunk_rows(site, rule, call, entry, index, name="chunk_rows"):
    for v, out in zip(CHUNK_VALUES, rule):
        expect = raises(ValueError, CHUNK_MSG % (name, out)) if isinstance(out, str) else arg(entry, index, out)
        row("%s-%s-%r" % (name, site, v), (lambda v=v: call(v)), expect)


_chunk_rows("GP.var", LENIENT, lambda v: _gp().var(_xo(3), chunk_rows=v), "gpx_gp_var", 3)
_chunk_rows("GP.dvar_dx", LENIENT, lambda v: _gp().dvar_dx(_xo(3), chunk_rows=v), "gpx_gp_var_grad", 3)
_chunk_rows("GP.predict_grad", LENIENT, lambda v: _gp().predict_grad(_xo(3), chunk_rows=v), "gpx_gp_var_grad", 3)
_chunk_rows("GP.loo", LENIENT, lambda v: _gp().loo(chunk_rows=v), "gpx_gp_loo", 1)
_chunk_rows("SparseGP.var", LENIENT, lambda v: _sgp().var(_xo(3), chunk_rows=v), "gpx_sgp_var", 3)
_chunk_rows("PosteriorPaths.call", STRICT, lambda v: _on_paths("__call__", _xo(3), v), "gpx_paths_eval", 3)
_chunk_rows("PosteriorPaths.grad", STRICT, lambda v: _on_paths("grad", _xo(3), v), "gpx_paths_grad", 3)
for _v, _out in zip(CHUNK_VALUES, LENIENT):
    row("chunk_cols-SparseGP-%r" % (_v,), (lambda v=_v: _sgp(chunk_cols=v).chunk_cols),
        raises(ValueError, CHUNK_MSG % ("chunk_cols", _out)) if isinstance(_out, str) else returns(_out))

# ---- seed ----
SEED_MSG = "invalid value for seed: %s (None, or an int in [0, 2**64))"
#: what ``seed=None`` draws after ``np.random.seed(3)``: two 32-bit draws from numpy's global state, the first one the high half
SEED_AFTER_3 = 0x8D01176A121B0698
SEEDS = [(0, 0), (2 ** 64 - 1, 2 ** 64 - 1), (2 ** 64, "18446744073709551616"), (-1, "-1"), (True, "True"), (1.5, "1.5")]


def _seeded(call):
    np.random.seed(3)
    return call()


for _site, _call, _entry, _index in (("GP.sample", lambda s: _gp().sample(_xo(3), seed=s), "gpx_gp_sample", 4),
                                     ("GP.sample_paths", lambda s: _gp().sample_paths(2, seed=s), "gpx_gp_paths_create", 3)):
    row("seed-%s-None" % _site, (lambda c=_call: _seeded(lambda: c(None))), arg(_entry, _index, SEED_AFTER_3))
    for _v, _out in SEEDS:
        row("seed-%s-%r" % (_site, _v), (lambda c=_call, v=_v: c(v)),
            raises(ValueError, SEED_MSG % _out) if isinstance(_out, str) else arg(_entry, _index, _out))

# ---- size and features ----
COUNT_MSG = "invalid value for %s: %s (%san int >= %d)"
for _v, _out in ((None, 1), (0, 0), (3, 3), (-1, "-1"), (True, "True"), (2.0, "2.0")):
    row("size-GP.sample-%r" % (_v,), (lambda v=_v: _gp().sample(_xo(3), size=v, seed=1)),
        raises(ValueError, COUNT_MSG % ("size", _out, "None, or ", 0)) if isinstance(_out, str) else arg("gpx_gp_sample", 3, _out))
for _v, _out in ((None, "None"), (0, 0), (3, 3), (-1, "-1"), (True, "True"), (2.0, "2.0")):
    row("size-GP.sample_paths-%r" % (_v,), (lambda v=_v: _gp().sample_paths(v, seed=1)),
        raises(ValueError, COUNT_MSG % ("size", _out, "", 0)) if isinstance(_out, str) else arg("gpx_gp_paths_create", 1, _out))
for _v, _out in ((None, "None"), (0, "0"), (3, 3), (-1, "-1"), (True, "True"), (2.0, "2.0")):
    row("features-GP.sample_paths-%r" % (_v,), (lambda v=_v: _gp().sample_paths(2, seed=1, features=v)),
        raises(ValueError, COUNT_MSG % ("features", _out, "", 1)) if isinstance(_out, str) else arg("gpx_gp_paths_create", 2, _out))

# ---- jitter and tol: a finite float >= 0, or None ----
K0_JITTER = float(np.sqrt(np.finfo(np.float64).eps) * gp.GaussianKernel(1.0, 1.0).diag(np.zeros((1, 3)))[0])     # sqrt(eps_dtype) * k(0)
for _v, _out in ((None, -1.0), (0.0, 0.0), (1e-6, 1e-6), (-1.0, "-1.0 (None, or a finite float"), (float("nan"), "nan (None, or a finite float"),
                 (float("inf"), "inf (None, or a finite float"), ("x", "'x' (None, or a float")):
    row("jitter-GP.sample-%r" % (_v,), (lambda v=_v: _gp().sample(_xo(3), seed=1, jitter=v)),
        raises(ValueError, "invalid value for jitter: %s >= 0)" % _out) if isinstance(_out, str) else arg("gpx_gp_sample", 6, _out))
NUMBER_MSG = "invalid value for %s: %s (None, or a finite number >= 0)"
for _v, _out in ((None, K0_JITTER), (0.0, 0.0), (1e-6, 1e-6), (-1.0, NUMBER_MSG % ("jitter", "-1.0")), (float("nan"), NUMBER_MSG % ("jitter", "nan")),
                 (float("inf"), NUMBER_MSG % ("jitter", "inf")), ("x", "could not convert string to float: 'x'")):
    row("jitter-SparseGP-%r" % (_v,), (lambda v=_v: _sgp(jitter=v).jitter), raises(ValueError, _out) if isinstance(_out, str) else returns(_out))
for _v, _out in ((None, K0_JITTER), (0.0, 0.0), (1e-6, 1e-6), (-1.0, NUMBER_MSG % ("tol", "-1.0")), (float("nan"), NUMBER_MSG % ("tol", "nan")),
                 (float("inf"), NUMBER_MSG % ("tol", "inf")), ("x", "could not convert string to float: 'x'")):
    row("tol-greedy_inducing-%r" % (_v,), (lambda v=_v: gp.SparseGP.greedy_inducing(gp.GaussianKernel(1.0, 1.0), _x(3), 4, tol=v)),
        raises(ValueError, _out) if isinstance(_out, str) else arg("gpx_sgp_select", 7, _out))

# ---- xo shapes at the three facades: (site, the call with xo, the entry an accepted xo reaches with m as argument 2) ----
XO_MSG = "invalid shape for xo: %s"
XO_SITES = (("GP", lambda d, xo: _gp(d).var(xo), "gpx_gp_var"),
            ("SparseGP", lambda d, xo: _sgp(d).var(xo), "gpx_sgp_var"),
            ("PosteriorPaths", lambda d, xo: _on_paths("__call__", xo, 0, 1 if d == "n1" else d, 1 if d == 1 else 2), "gpx_paths_eval"))
for _site, _call, _entry in XO_SITES:
    for _name, _d, _xo_val, _out in (
            ("m_for_d3", 3, np.zeros(4), "(4,)"), ("m_d", 3, np.zeros((4, 3)), 4), ("m_d_plus_1", 3, np.zeros((4, 4)), "(4, 4)"),
            ("3d", 3, np.zeros((2, 3, 1)), "(2, 3, 1)"), ("m_for_1d_x", 1, np.zeros(5), 5), ("m_1_for_1d_x", 1, np.zeros((5, 1)), 5),
            ("m_for_n_by_1_x", "n1", np.zeros(5), "(5,)" if _site == "PosteriorPaths" else 5), ("m_1_for_n_by_1_x", "n1", np.zeros((5, 1)), 5)):
        row("xo-%s-%s" % (_site, _name), (lambda c=_call, d=_d, xo=_xo_val: c(d, xo)),
            raises(ValueError, XO_MSG % _out) if isinstance(_out, str) else arg(_entry, 2, _out))
    # a 0-d xo is one point to all three: numpy.ascontiguousarray hands back (1,) for it
    row("xo-%s-0d_for_d3" % _site, (lambda c=_call: c(3, np.float64(1.0))), raises(ValueError, XO_MSG % "(1,)"))
    row("xo-%s-0d_for_1d_x" % _site, (lambda c=_call: c(1, np.float64(1.0))), arg(_entry, 2, 1))

# ---- kernel eligibility: the route of every derivative member, every family x d in (1, 3), and a plugin kernel ----
NO_ARD = "%s is not implemented for GaussianARDKernel (dloglh_dtheta and dlh_dtheta are)"
NEEDS_BUILTIN = raises(NotImplementedError, "d2loglh_dtheta2 needs a built-in kernel (periodic: 1-D inputs)")
NO_DKDX = raises(NotImplementedError, "dmean_dx needs a built-in kernel: the kernel plugin contract (K, jacobian, hessian) has no "
                                      "derivative with respect to the inputs, dk/dx")
NO_PATHS = "sample_paths supports GaussianKernel and GaussianARDKernel (a random-feature prior needs the kernel's spectral density); %s is not supported"
HOST = "gpx_gp_get_inv_Kxx"           # the host routes begin with the download of the explicit inverse
MEMBERS = {           # member: (how it is called, the device entry, {family: (what happens at d = 1, at d = 3)}; "device" / an entry / a refusal)
    "dloglh_dtheta": (lambda g, xo: g.dloglh_dtheta, "gpx_gp_dloglh_dtheta",
                      {"gaussian": ("device", "device"), "periodic": ("device", HOST), "ard": ("device", "device"), "plugin": (HOST, HOST)}),
    "dloo_dtheta": (lambda g, xo: g.dloo_dtheta, "gpx_gp_loo_grad",
                    {"gaussian": ("device", "device"), "periodic": ("device", "gpx_gp_loo_grad_weights"), "ard": ("device", "device"),
                     "plugin": ("gpx_gp_loo_grad_weights",) * 2}),
    "d2lh_dtheta2": (lambda g, xo: g.d2lh_dtheta2, "gpx_gp_dlh_d2lh",
                     {"gaussian": ("device", "device"), "periodic": ("device", HOST),
                      "ard": (raises(NotImplementedError, NO_ARD % "d2lh_dtheta2"),) * 2, "plugin": (HOST, HOST)}),
    "d2loglh_dtheta2": (lambda g, xo: g.d2loglh_dtheta2, "gpx_gp_dlh_d2lh",
                        {"gaussian": ("device", "device"), "periodic": ("device", NEEDS_BUILTIN),
                         "ard": (raises(NotImplementedError, NO_ARD % "d2loglh_dtheta2"),) * 2, "plugin": (NEEDS_BUILTIN, NEEDS_BUILTIN)}),
    "dm_dtheta": (lambda g, xo: g.dm_dtheta(xo), "gpx_gp_dm_dtheta",
                  {"gaussian": ("device", "device"), "periodic": ("device", HOST),
                   "ard": (raises(NotImplementedError, NO_ARD % "dm_dtheta"),) * 2, "plugin": (HOST, HOST)}),
    "dmean_dx": (lambda g, xo: g.dmean_dx(xo), "gpx_gp_mean_grad",
                 {"gaussian": ("device", "device"), "periodic": ("device", "device"), "ard": ("device", "device"), "plugin": (NO_DKDX, NO_DKDX)}),
    "sample_paths": (lambda g, xo: g.sample_paths(2, seed=1), "gpx_gp_paths_create",
                     {"gaussian": ("device", "device"), "periodic": (raises(NotImplementedError, NO_PATHS % "PeriodicKernel"),) * 2,
                      "ard": ("device", "device"), "plugin": (raises(NotImplementedError, NO_PATHS % "_Plugin"),) * 2}),
}


def _route(lib, call, expect):
    """A refusal as in `_check`; otherwise the first entry of `STOPS` the member calls is the route it took."""
    if isinstance(expect, tuple):
        return _check(lib, call, expect)
    with pytest.raises(Reached) as r:
        call()
    assert r.value.entry == expect


ROUTES = [pytest.param(call, dev if out == "device" else out, family, d, id="%s-%s-d%d" % (member, family, d))
          for member, (call, dev, table) in MEMBERS.items() for family, pair in table.items() for d, out in zip((1, 3), pair)]


@pytest.mark.parametrize("call,expect,family,d", ROUTES)
def test_route_of_every_member_by_kernel_family(lib, call, expect, family, d):
    g = _gp(d, family)
    _route(lib, lambda: call(g, _xo(d)), expect)


def test_a_kernel_swapped_after_construction_is_followed(lib):
    g = _gp(3)
    g.K = _Plugin(1.0, 1.0)
    _check(lib, lambda: g.dmean_dx(_xo(3)), NO_DKDX)
    g.K = gp.GaussianARDKernel(1.0, [1.0, 2.0, 3.0])
    _route(lib, lambda: g.dmean_dx(_xo(3)), "gpx_gp_mean_grad")
    _check(lib, lambda: g.d2lh_dtheta2, raises(NotImplementedError, NO_ARD % "d2lh_dtheta2"))


# ---- the refusing wrappers keep their own exception types and texts ----
ARD2 = lambda: gp.GaussianARDKernel(1.0, [1.0, 2.0])            # noqa: E731 -- two widths against three input dimensions
WIDTHS = "x has 3 dimension(s), the kernel has 2 width(s)"
row("plugin-SparseGP", lambda: _sgp(K=_Plugin(1.0, 1.0)),
    raises(NotImplementedError, "SparseGP needs a built-in kernel (GaussianKernel, PeriodicKernel, GaussianARDKernel): plugin kernels are not supported"))
row("plugin-greedy_inducing", lambda: gp.SparseGP.greedy_inducing(_Plugin(1.0, 1.0), _x(3), 4),
    raises(NotImplementedError, "SparseGP needs a built-in kernel (GaussianKernel, PeriodicKernel, GaussianARDKernel): plugin kernels are not supported"))
row("ard_widths-SparseGP", lambda: _sgp(K=ARD2()).elbo, raises(ValueError, WIDTHS))
row("ard_widths-greedy_inducing", lambda: gp.SparseGP.greedy_inducing(ARD2(), _x(3), 4), raises(ValueError, WIDTHS))
row("ard_widths-GP", lambda: gp.GP(ARD2(), _x(3), Y, s=1.0).log_lh, raises(ValueError, WIDTHS))
row("ard-SparseGP", lambda: _sgp(K=gp.GaussianARDKernel(1.0, [1.0, 2.0, 3.0])).elbo, arg("gpx_sgp_create", 2, _lib.KERNEL_GAUSSIAN_ARD))
row("plugin-DistributedGP", lambda: gp.DistributedGP(_Plugin(1.0, 1.0), _x(3), Y, s=1.0),
    raises(TypeError, "DistributedGP needs a built-in kernel (GaussianKernel or PeriodicKernel); _Plugin is a Python kernel plugin, which gp.GP "
                      "supports on one GPU"))
row("ard-DistributedGP", lambda: gp.DistributedGP(gp.GaussianARDKernel(1.0, [1.0, 2.0, 3.0]), _x(3), Y, s=1.0),
    raises(NotImplementedError, "DistributedGP does not support GaussianARDKernel: the multi-GPU fit knows GaussianKernel and PeriodicKernel only; "
                                "gp.GP has the ARD family on one GPU"))

# ---- the dtype table ----
SPELLINGS = (("float64", _lib.F64), ("f64", _lib.F64), (np.float64, _lib.F64), ("float32", _lib.F32), ("f32", _lib.F32), (np.float32, _lib.F32))
_TH = np.ones((2, 3))
DTYPE_SITES = (("GP", lambda dt: _gp(dtype=dt)._dtype, None, None),
               ("SparseGP", lambda dt: _sgp(dtype=dt)._dtype, None, None),
               ("greedy_inducing", lambda dt: gp.SparseGP.greedy_inducing(gp.GaussianKernel(1.0, 1.0), _x(3), 4, dtype=dt), "gpx_sgp_select", 0))
for _site, _call, _entry, _index in DTYPE_SITES:
    for _dt, _id in SPELLINGS:
        row("dtype-%s-%s" % (_site, getattr(_dt, "__name__", _dt)), (lambda c=_call, dt=_dt: c(dt)), arg(_entry, _index, _id) if _entry else returns(_id))
    row("dtype-%s-unknown" % _site, (lambda c=_call: c("double")), raises(KeyError, "'double'"))
MLII_SITES = (("BatchEvaluator", lambda dt: mlii.BatchEvaluator(_x(3), Y, dtype=dt)),
              ("log_lh_batch", lambda dt: mlii.log_lh_batch(_x(3), Y, _TH, dtype=dt)),
              ("log_lh_batch_rows", lambda dt: mlii.log_lh_batch(_x(3), Y, _TH, dtype=dt, batched=False)))
for _site, _call in MLII_SITES:
    for _dt, _id in SPELLINGS:
        # CHANGED: `mlii` compared with ("float64", "f64") and ran everything else -- numpy.float64 too -- in fp32
        row("dtype-%s-%s%s" % (_site, getattr(_dt, "__name__", _dt), "-CHANGED" if _dt is np.float64 else ""), (lambda c=_call, dt=_dt: c(dt)),
            arg("gpx_gp_create", 1, _id))
    # CHANGED: ... and so did an unknown value, without a word
    row("dtype-%s-unknown-CHANGED" % _site, (lambda c=_call: c("double")), raises(KeyError, "'double'"))


@pytest.mark.parametrize("call,expect", ROWS)
def test_argument_rule(lib, call, expect):
    if expect[0] == "arg" and expect[1] in ("gpx_gp_create", "gpx_sgp_create"):       # (every fit passes these: they stop only these rows)
        lib.stops = {expect[1]}
    _check(lib, call, expect)


def test_seed_none_restated():
    r = np.random.RandomState(3)
    assert SEED_AFTER_3 == int(r.randint(0, 2 ** 32)) << 32 | int(r.randint(0, 2 ** 32))
