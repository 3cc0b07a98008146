"""tools/extend_bench.py -- time gpx_gp_extend against the refit it replaces (profiles/extend_bench_*.json).

    python tools/extend_bench.py [--n 8192] [--d 32] [--ks 1,64,1024] [--repeats 10] [--step-timeout 300]
    python tools/extend_bench.py --schur-only [--lib PATH] ...      only (d), optionally on another build of the library

One process, one JSON object on stdout; fp64 Gaussian.  One fitted source handle of n points; per k a second handle of
n + k points that is refitted (gpx_gp_fit: untouched by GP.extend, so its time is what taking the k points in cost
before).  Every GPU step runs under a watchdog of its own (--step-timeout seconds): a step that overruns it ends the
process with exit status 124, so nothing further is started on the device.  Times are a host clock around the synchronous
calls, after a warm-up of the same shape, the two calls ALTERNATING so that both see the same state of the machine.  The
extended handle is destroyed outside the timed region.

  (a) extend and refit in ms (median, min, max, all runs) and their ratio
  (b) the stages of the last extend (gpx_gp_last_timing of the new handle) and of the last refit
  (c) the gpx_prof split of one extend: every launch class, and for the two new kernels (class 13) launches, ms, bytes
      and bytes/s -- HIP events around each launch
  (d) gpx_d_schur_lower alone on a k x n block, the figure behind its slice width
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
        "gemm_panel_bn128", "gemm_trailing_bn64", "transpose", "pred_grad", "extend"]
STAGES = ("rows_of_K", "copy_sweep_schur_potrf", "solves", "reductions", "total")
FIT_STAGES = ("kernel_build", "potrf", "solve", "reduce", "total")


class Step(object):
    """A GPU step under its own time limit: the process exits (status 124) when the step overruns it."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        sys.stderr.write("[extend_bench] %s\n" % self.name)
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


def timing(handle, names):
    ms = (ctypes.c_float * 5)()
    _lib.check(_lib.load().gpx_gp_last_timing(handle, ms))
    return dict(zip(names, [round(float(v), 4) for v in ms]))


def prof_read():
    lib, out = _lib.load(), {}
    for cls, name in enumerate(PROF):
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _lib.check(lib.gpx_prof_read(cls, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        if a.value:
            out[name] = {"launches": a.value, "ms": b.value, "work": c.value}
    return out


def schur_alone(k, n, repeats):
    """ms of gpx_d_schur_lower on a k x n block of zeros (S is overwritten every time: the values do not matter)."""
    lib = _lib.load()
    ldb, lds = -(-n // 16) * 16, -(-k // 16) * 16
    B, S = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.gpx_malloc(ctypes.byref(B), k * ldb * 8))
    _lib.check(lib.gpx_malloc(ctypes.byref(S), k * lds * 8))
    try:
        _lib.check(lib.gpx_memset(B, 0, k * ldb * 8, None))
        _lib.check(lib.gpx_memset(S, 0, k * lds * 8, None))
        ms = []
        for i in range(repeats + 2):
            _lib.check(lib.gpx_device_sync())
            t0 = time.perf_counter()
            _lib.check(lib.gpx_d_schur_lower(_lib.F64, B, k, n, ldb, S, lds, None))
            _lib.check(lib.gpx_device_sync())
            if i >= 2:
                ms.append((time.perf_counter() - t0) * 1e3)
    finally:
        lib.gpx_free(B)
        lib.gpx_free(S)
    return stats(ms)


def one_k(g, X, y, n, k, args):
    lib = _lib.load()
    src = g._fit_pd().handle
    xn, yn = np.ascontiguousarray(X[n:n + k]), np.ascontiguousarray(y[n:n + k])
    res = {"k": k}
    refit = gp.GP(gp.GaussianKernel(*g.K.params), X[:n + k], y[:n + k], s=1.0)
    info = ctypes.c_int(0)

    def extend(keep=False):
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        _lib.check(lib.gpx_gp_extend(src, _lib.dptr(xn), _lib.dptr(yn), k, ctypes.byref(h), ctypes.byref(info)))
        ms = (time.perf_counter() - t0) * 1e3
        if keep:
            return ms, h
        lib.gpx_gp_destroy(h)
        return ms, None

    with Step("refit handle n + k = %d" % (n + k), args.step_timeout):
        st = refit._fit_pd()                               # warm-up of the refit (and its data upload)
        res["log_lh_refit"] = float(refit.log_lh)

    def fit():
        t0 = time.perf_counter()
        _lib.check(lib.gpx_gp_fit(st.handle, ctypes.byref(info)))
        return (time.perf_counter() - t0) * 1e3

    with Step("warm-up and timing n = %d k = %d" % (n, k), args.step_timeout):
        extend()
        e_ms, f_ms = [], []
        for _ in range(args.repeats):
            e_ms.append(extend()[0])
            f_ms.append(fit())
        res["extend"], res["refit"] = stats(e_ms), stats(f_ms)
        res["refit_over_extend"] = res["refit"]["median_ms"] / res["extend"]["median_ms"]
        res["refit_stages_ms"] = timing(st.handle, FIT_STAGES)
        _, h = extend(keep=True)
        try:
            res["extend_stages_ms"] = timing(h, STAGES)
            llh = ctypes.c_double(0.0)
            _lib.check(lib.gpx_gp_log_lh(h, ctypes.byref(llh)))
            res["log_lh_extend"] = llh.value
        finally:
            lib.gpx_gp_destroy(h)
    with Step("gpx_prof split n = %d k = %d" % (n, k), args.step_timeout):
        _lib.check(lib.gpx_prof_enable(1))
        extend()
        res["prof"] = prof_read()
        _lib.check(lib.gpx_prof_enable(0))
        ex = res["prof"].get("extend")
        if ex:
            ex["bytes_per_s"] = ex["work"] / (ex["ms"] * 1e-3)
    with Step("schur alone k = %d n = %d" % (k, n), args.step_timeout):
        res["schur_alone"] = schur_alone(k, n, args.repeats)
    refit._dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--ks", default="1,64,1024")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--schur-only", action="store_true", help="time gpx_d_schur_lower alone")
    ap.add_argument("--lib", default=None, help="another build of libgpx.so (SCHUR_MIN_SLICE / SCHUR_TARGET_WGS of "
                                                "csrc/gpx_extend.hip edited, `make`, the library copied aside)")
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    n, d = args.n, args.d
    ks = [int(v) for v in args.ks.split(",")]
    if args.schur_only:
        out = {"lib": os.path.basename(_lib.LIB_PATH), "n": n, "dtype": "float64", "schur_alone": {}}
        for k in ks:
            with Step("schur alone k = %d n = %d" % (k, n), args.step_timeout):
                out["schur_alone"][str(k)] = schur_alone(k, n, args.repeats)
        print(json.dumps(out))
        return
    rng = np.random.RandomState(0)
    X = rng.uniform(-10, 10, (n + max(ks), d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(n + max(ks))
    res = {"device": _lib.device_info(0)["name"], "n": n, "d": d, "dtype": "float64", "kernel": "gaussian", "s": 1.0,
           "repeats": args.repeats,
           "clock": "host perf_counter around the synchronous calls, extend and refit alternating; stages: HIP events on the "
                    "handle's stream; gpx_prof: HIP events around each launch", "ks": []}
    g = gp.GP(gp.GaussianKernel(1.0, 0.5 * np.sqrt(d)), X[:n], y[:n], s=1.0)
    with Step("fit n = %d" % n, args.step_timeout):
        t0 = time.perf_counter()
        res["log_lh"] = float(g.log_lh)
        res["first_fit_s"] = time.perf_counter() - t0
    for k in ks:
        res["ks"].append(one_k(g, X, y, n, k, args))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
