"""tools/xgrad_bench.py -- time the input-space gradients against GP.var / GP.mean on the same handle (DESIGN section 4,
profiles/xgrad_bench.json).

    python tools/xgrad_bench.py [--sizes 8192:3:1024,65536:32:1000] [--repeats 5] [--step-timeout 300]

One process, one JSON object on stdout; one fitted handle per size (N:d:m).  Every GPU step runs under a watchdog of its
own (--step-timeout seconds): a step that overruns it ends the process with exit status 124, so nothing further is
started on the device.  Times are a host clock around calls that end in a download (they synchronise), after a warm-up,
with the calls ALTERNATING so that all see the same state of the machine.

  (a) var, dvar_dx and predict_grad in ms, and dvar_dx / var (the yardstick: by flops two sweeps against one, about 2 x)
  (b) mean against dmean_dx
  (c) the gpx_prof split of one var and one dvar_dx call: products (forward sweep = the var call's, backward sweep = the
      difference), in-block substitutions, panel transposes, the fused gradient pass, kernel build
"""
import argparse
import ctypes
import faulthandler
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_processes_amd as gp                      # noqa: E402
from gaussian_processes_amd import _lib                  # noqa: E402

PROF = ["kmat", "gemm_trailing", "potrf_diag", "trsm_rows", "trsv", "mean", "reduce", "gemm_panel_bn64", "gemm_generic",
        "gemm_panel_bn128", "gemm_trailing_bn64", "transpose", "pred_grad"]
GEMMS = ("gemm_trailing", "gemm_panel_bn64", "gemm_generic", "gemm_panel_bn128", "gemm_trailing_bn64")


class Step(object):
    """A GPU step under its own time limit: the process exits (status 124) when the step overruns it."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        sys.stderr.write("[xgrad_bench] %s\n" % self.name)
        sys.stderr.flush()
        faulthandler.dump_traceback_later(self.seconds, exit=False, file=sys.stderr)
        self._t = threading.Timer(self.seconds + 1.0, lambda: os._exit(124))
        self._t.daemon = True
        self._t.start()
        return self

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()
        self._t.cancel()
        return False


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs_ms": [round(v, 3) for v in ms]}


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def profiled(f):
    """{class: ms} of the launches of one call (HIP events around every launch: the sum, not the wall time)."""
    lib = _lib.load()
    _lib.check(lib.gpx_prof_enable(1))
    f()
    out = {}
    for cls, name in enumerate(PROF):
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _lib.check(lib.gpx_prof_read(cls, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        if a.value:
            out[name] = {"launches": a.value, "ms": b.value}
    _lib.check(lib.gpx_prof_enable(0))
    return out


def one_size(N, d, m, args):
    rng = np.random.RandomState(0)
    X = rng.uniform(-10, 10, (N, d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(N)
    Xo = np.random.RandomState(1).uniform(-10, 10, (m, d))
    res = {"n": N, "d": d, "m": m, "dtype": "float64", "s": 1.0, "chunks": _lib.var_plan(_lib.F64, N, m)[1]}
    g = gp.GP(gp.GaussianKernel(1.0, 0.5 * np.sqrt(d)), X, y, s=1.0)
    with Step("fit N = %d" % N, args.step_timeout):
        t0 = time.perf_counter()
        res["log_lh"] = float(g.log_lh)
        res["fit_s"] = time.perf_counter() - t0
    calls = {"var": lambda: g.var(Xo), "dvar_dx": lambda: g.dvar_dx(Xo), "predict_grad": lambda: g.predict_grad(Xo),
             "mean": lambda: g.mean(Xo), "dmean_dx": lambda: g.dmean_dx(Xo)}
    with Step("warm-up and timing N = %d m = %d" % (N, m), args.step_timeout):
        for f in calls.values():
            f()
        ms = {k: [] for k in calls}
        for _ in range(args.repeats):
            for k, f in calls.items():
                ms[k].append(timed(f))
        res["ms"] = {k: stats(v) for k, v in ms.items()}
        res["dvar_dx_over_var"] = res["ms"]["dvar_dx"]["median_ms"] / res["ms"]["var"]["median_ms"]
        res["dmean_dx_over_mean"] = res["ms"]["dmean_dx"]["median_ms"] / res["ms"]["mean"]["median_ms"]
    with Step("gpx_prof split N = %d" % N, args.step_timeout):
        pv, pg = profiled(calls["var"]), profiled(calls["dvar_dx"])
        gemm = lambda p: sum(p.get(k, {"ms": 0.0})["ms"] for k in GEMMS)   # noqa: E731
        get = lambda p, k: p.get(k, {"ms": 0.0})["ms"]                     # noqa: E731
        res["prof"] = {"var": pv, "dvar_dx": pg}
        res["split_ms"] = {
            "kernel_build": get(pg, "kmat"),
            "forward_sweep_products": gemm(pv),
            "backward_sweep_products": gemm(pg) - gemm(pv),
            "in_block_substitutions": get(pg, "trsm_rows"),
            "panel_transposes": get(pg, "transpose"),
            "fused_gradient_pass": get(pg, "pred_grad"),
        }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192:3:1024,65536:32:1000", help="comma-separated N:d:m")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    args = ap.parse_args()
    res = {"device": _lib.device_info(0)["name"], "repeats": args.repeats,
           "clock": "host perf_counter around calls that end in a download; gpx_prof: HIP events around each launch", "sizes": []}
    for spec in args.sizes.split(","):
        N, d, m = (int(v) for v in spec.split(":"))
        res["sizes"].append(one_size(N, d, m, args))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
