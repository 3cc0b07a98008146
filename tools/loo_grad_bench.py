"""tools/loo_grad_bench.py -- time GP.dloo_dtheta against GP.dloglh_dtheta (profiles/loo_grad_bench_*.json).

    python tools/loo_grad_bench.py [--sizes 2048,8192,16384] [--d 8[,32]] [--kernels gaussian[,ard]] [--dtypes float64,float32]
                                   [--repeats 7] [--batch-n 2048] [--step-timeout 300] [--out profiles/loo_grad_bench_<date>.json]

One process, one JSON object (stdout, and the file).  Per (kernel, n, d, dtype) ONE fitted handle; on it
gpx_gp_loo_grad and gpx_gp_dloglh_dtheta ALTERNATE, so that both see the same state of the machine, after a warm-up of each.
Both calls are synchronous (they end with a wait for the handle's stream and a host sum of the partials): the clock is the
host's around the call.  The median of the repeats is reported beside min, max and every run.  Then, in a pass of its own,
the gpx_prof split of --repeats calls each, again alternating: HIP events around every launch, by launch class; the first
call's split is reported whole, and the device time of the fused reduction (class `reduce`: tile_reduce_kernel /
tile_reduce_ard_kernel alone) for every repeat as `reduce_*`.  To compare two builds of the library run the tool once per
build, the builds alternating, and set the `reduce_*` medians of one against the run-to-run range of the other.
The flop count predicts one more n^3 product for the leave-one-out gradient (K^-1 whole instead of its lower triangle, and P = Y Y^T): `loo_over_loglh`.
Last, gpx_gp_fit_batch_loo against gpx_gp_fit_batch_grad for the same 8 rows at --batch-n.
Every GPU step runs under a watchdog of its own (--step-timeout seconds): a step that overruns it ends the process with
exit status 124, so nothing further is started on the device.
"""
import argparse
import ctypes
import datetime
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
from gaussian_processes_amd import _lib, mlii            # noqa: E402

PROF = ["kmat", "gemm_trailing", "potrf_diag", "trsm_rows", "trsv", "mean", "reduce", "gemm_panel_bn64", "gemm_generic",
        "gemm_panel_bn128", "gemm_trailing_bn64", "transpose", "pred_grad", "extend", "randn", "rff", "kapply", "kapply_grad",
        "chol_delete"]


class Step(object):
    """A GPU step under its own time limit: the process exits (status 124) when the step overruns it."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        sys.stderr.write("[loo_grad_bench] %s\n" % self.name)
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


def prof_of(call):
    lib, out = _lib.load(), {}
    _lib.check(lib.gpx_prof_enable(1))                     # (also clears the registry)
    call()
    for cls, name in enumerate(PROF):
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _lib.check(lib.gpx_prof_read(cls, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        if a.value:
            out[name] = {"launches": a.value, "ms": round(b.value, 4)}
    _lib.check(lib.gpx_prof_enable(0))
    return out


def data(n, d):
    rng = np.random.RandomState(0)
    X = rng.uniform(-10, 10, (n, d))
    return X, np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(n)


def one_size(n, d, dtype, kernel, args):
    lib = _lib.load()
    X, y = data(n, d)
    if kernel == "ard":
        k = gp.GaussianARDKernel(1.0, 0.5 * np.sqrt(d) * np.random.RandomState(7).uniform(0.5, 2.0, d))
    else:
        k = gp.GaussianKernel(1.0, 0.5 * np.sqrt(d))
    g = gp.GP(k, X, y, s=1.0, dtype=dtype)
    res = {"kernel": kernel, "n": n, "d": d, "dtype": dtype}
    with Step("fit n = %d %s" % (n, dtype), args.step_timeout):
        h = g._fit_pd().handle
        res["log_lh"] = float(g.log_lh)
    out, val = np.empty(len(g.params)), ctypes.c_double(0.0)

    def loo():
        t0 = time.perf_counter()
        _lib.check(lib.gpx_gp_loo_grad(h, ctypes.byref(val), _lib.dptr(out)))
        return (time.perf_counter() - t0) * 1e3

    def llh():
        t0 = time.perf_counter()
        _lib.check(lib.gpx_gp_dloglh_dtheta(h, _lib.dptr(out)))
        return (time.perf_counter() - t0) * 1e3

    with Step("warm-up and timing n = %d %s" % (n, dtype), args.step_timeout):
        loo(), llh()
        a, b = [], []
        for _ in range(args.repeats):
            a.append(loo())
            b.append(llh())
        res["dloo_dtheta"], res["dloglh_dtheta"] = stats(a), stats(b)
        res["loo_over_loglh"] = res["dloo_dtheta"]["median_ms"] / res["dloglh_dtheta"]["median_ms"]
        res["loo_log_lh"] = val.value
    with Step("gpx_prof split n = %d %s" % (n, dtype), args.step_timeout):
        a, b = [], []
        for _ in range(args.repeats):
            a.append(prof_of(loo))
            b.append(prof_of(llh))
        res["prof_dloo_dtheta"], res["prof_dloglh_dtheta"] = a[0], b[0]
        res["reduce_dloo_dtheta"] = stats([p["reduce"]["ms"] for p in a])
        res["reduce_dloglh_dtheta"] = stats([p["reduce"]["ms"] for p in b])
    g._dev.close()
    return res


def batch(n, d, args):
    X, y = data(n, d)
    rs = np.random.RandomState(1)
    th = np.column_stack([rs.uniform(0.5, 2.0, 8), rs.uniform(0.5, 2.0, 8) * 0.5 * np.sqrt(d), rs.uniform(0.5, 1.5, 8)])
    res = {"n": n, "d": d, "dtype": "float64", "rows": 8}
    with mlii.BatchEvaluator(X, y) as ev:
        def run(criterion):
            t0 = time.perf_counter()
            ev.value_and_grad(th, criterion=criterion)
            return (time.perf_counter() - t0) * 1e3
        with Step("fit_batch warm-up and timing n = %d" % n, args.step_timeout):
            run("loo"), run("log_lh")
            a, b = [], []
            for _ in range(args.repeats):
                a.append(run("loo"))
                b.append(run("log_lh"))
    res["fit_batch_loo"], res["fit_batch_grad"] = stats(a), stats(b)
    res["loo_over_loglh"] = res["fit_batch_loo"]["median_ms"] / res["fit_batch_grad"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,8192,16384")
    ap.add_argument("--d", default="8", help="input dimensions, comma separated (the batch uses the first)")
    ap.add_argument("--kernels", default="gaussian", help="gaussian,ard")
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch-n", type=int, default=2048)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ds = [int(v) for v in args.d.split(",") if v]
    res = {"device": _lib.device_info(0)["name"], "kernels": args.kernels, "s": 1.0, "repeats": args.repeats,
           "clock": "host perf_counter around the synchronous calls, the two gradients alternating on one fitted handle, after "
                    "one warm-up call each; prof_*, reduce_*: gpx_prof, HIP events around each launch, in a pass of its own",
           "sizes": [], "batch": None}
    for kernel in args.kernels.split(","):
        for n in [int(v) for v in args.sizes.split(",") if v]:
            for d in ds:
                for dtype in args.dtypes.split(","):
                    res["sizes"].append(one_size(n, d, dtype, kernel, args))
    if args.batch_n > 0:
        res["batch"] = batch(args.batch_n, ds[0], args)
    text = json.dumps(res)
    path = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                    "loo_grad_bench_%s.json" % datetime.date.today().isoformat())
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
