"""tools/remove_bench.py -- time gpx_gp_remove against the refit it replaces (profiles/remove_bench_*.json).

    python tools/remove_bench.py [--n 8192] [--d 32] [--cases first,last,oldest16,random16,oldest256] [--repeats 10] [--step-timeout 300]
                                 [--lib PATH]      another build of the library (DEL_W / DEL_G / DEL_ROWS of csrc/gpx_remove.hip edited)

One process, one JSON object on stdout; fp64 Gaussian.  One fitted source handle of n points; per case a second handle on
the kept points that is refitted (gpx_gp_fit: untouched by GP.remove, so its time is what dropping the points cost before).
Every GPU step runs under a watchdog of its own (--step-timeout seconds): a step that overruns it ends the process with
exit status 124, so nothing further is started on the device.  Times are a host clock around the synchronous calls, after
a warm-up of the same shape, the two calls ALTERNATING so that both see the same state of the machine.  The shrunk handle
is destroyed outside the timed region.

  (a) remove and refit in ms (median, min, max, all runs) and their ratio
  (b) the stages of the last remove (gpx_gp_last_timing of the new handle) and of the last refit
  (c) the gpx_prof split of one remove: every launch class, and for the deletion launches (class 18) ms, bytes and
      bytes/s -- one pair of HIP events around all of them
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
        "gemm_panel_bn128", "gemm_trailing_bn64", "transpose", "pred_grad", "extend", "randn", "rff", "kapply", "kapply_grad",
        "chol_delete"]
STAGES = ("nothing", "deletion", "solves", "reductions", "total")
FIT_STAGES = ("kernel_build", "potrf", "solve", "reduce", "total")


class Step(object):
    """A GPU step under its own time limit: the process exits (status 124) when the step overruns it."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        sys.stderr.write("[remove_bench] %s\n" % self.name)
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


def indices(name, n):
    if name == "first":
        return [0]
    if name == "last":
        return [n - 1]
    if name.startswith("oldest"):
        return list(range(int(name[6:])))
    if name.startswith("random"):
        return sorted(int(i) for i in np.random.RandomState(1).choice(n, int(name[6:]), replace=False))
    raise SystemExit("unknown case %r" % name)


def one_case(g, X, y, n, name, args):
    lib = _lib.load()
    src = g._fit_pd().handle
    idx = np.ascontiguousarray(indices(name, n), dtype=np.int64)
    k, ip = len(idx), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    res = {"case": name, "k": k, "first_index": int(idx[0])}
    refit = gp.GP(gp.GaussianKernel(*g.K.params), np.delete(X, idx, axis=0), np.delete(y, idx), s=1.0)
    info = ctypes.c_int(0)

    def remove(keep=False):
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        _lib.check(lib.gpx_gp_remove(src, ip, k, ctypes.byref(h), ctypes.byref(info)))
        ms = (time.perf_counter() - t0) * 1e3
        if keep:
            return ms, h
        lib.gpx_gp_destroy(h)
        return ms, None

    with Step("refit handle n - k = %d" % (n - k), args.step_timeout):
        st = refit._fit_pd()                               # warm-up of the refit (and its data upload)
        res["log_lh_refit"] = float(refit.log_lh)

    def fit():
        t0 = time.perf_counter()
        _lib.check(lib.gpx_gp_fit(st.handle, ctypes.byref(info)))
        return (time.perf_counter() - t0) * 1e3

    with Step("warm-up and timing n = %d case %s" % (n, name), args.step_timeout):
        remove()
        r_ms, f_ms = [], []
        for _ in range(args.repeats):
            r_ms.append(remove()[0])
            f_ms.append(fit())
        res["remove"], res["refit"] = stats(r_ms), stats(f_ms)
        res["refit_over_remove"] = res["refit"]["median_ms"] / res["remove"]["median_ms"]
        res["refit_stages_ms"] = timing(st.handle, FIT_STAGES)
        _, h = remove(keep=True)
        try:
            res["remove_stages_ms"] = timing(h, STAGES)
            llh = ctypes.c_double(0.0)
            _lib.check(lib.gpx_gp_log_lh(h, ctypes.byref(llh)))
            res["log_lh_remove"] = llh.value
        finally:
            lib.gpx_gp_destroy(h)
    with Step("gpx_prof split n = %d case %s" % (n, name), args.step_timeout):
        _lib.check(lib.gpx_prof_enable(1))
        remove()
        res["prof"] = prof_read()
        _lib.check(lib.gpx_prof_enable(0))
        de = res["prof"].get("chol_delete")
        if de:
            de["bytes_per_s"] = de["work"] / (de["ms"] * 1e-3)
    refit._dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--cases", default="first,last,oldest16,random16,oldest256")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--lib", default=None, help="another build of libgpx.so (the constants of csrc/gpx_remove.hip edited, "
                                                "`make`, the library copied aside)")
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    n, d = args.n, args.d
    rng = np.random.RandomState(0)
    X = rng.uniform(-10, 10, (n, d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(n)
    res = {"lib": os.path.basename(_lib.LIB_PATH), "device": _lib.device_info(0)["name"], "n": n, "d": d, "dtype": "float64", "kernel": "gaussian", "s": 1.0,
           "repeats": args.repeats,
           "clock": "host perf_counter around the synchronous calls, remove and refit alternating; stages: HIP events on the "
                    "handle's stream; gpx_prof: HIP events around each launch, ONE pair around all deletion launches",
           "cases": []}
    g = gp.GP(gp.GaussianKernel(1.0, 0.5 * np.sqrt(d)), X, y, s=1.0)
    with Step("fit n = %d" % n, args.step_timeout):
        t0 = time.perf_counter()
        res["log_lh"] = float(g.log_lh)
        res["first_fit_s"] = time.perf_counter() - t0
    for name in args.cases.split(","):
        res["cases"].append(one_case(g, X, y, n, name, args))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
