"""tools/sample_bench.py -- time GP.sample against the host route it replaces (profiles/sample_bench_*.json).

    python tools/sample_bench.py [--n 8192] [--d 8] [--ms 1024,4096] [--size 64] [--repeats 7] [--warmup 2] [--step-timeout 300]

One process, one JSON object on stdout and in profiles/sample_bench_n<n>.json (--out); fp64 Gaussian, s = 1.  One fitted GP
of n points; per m the two routes from that GP to `size` joint draws at m test points:

  device   g.sample(xo, size, seed)                 covariance, factor, normals and product in HBM; size x m comes back
  host     C = g.cov(xo); L = numpy.linalg.cholesky(C + jitter I); f = g.mean(xo) + z @ L.T      (the same jitter; z from numpy)

Every GPU step runs under a watchdog of its own (--step-timeout seconds): a step that overruns it ends the process with exit
status 124, so nothing further is started on the device.  Times are a host clock around the synchronous calls, after
warm-up runs of the same shape, the two routes ALTERNATING so that both see the same state of the machine; medians are
reported with min, max and every run.  The host route is split into its three parts (cov with its download, the
factorisation, mean + product).  gpx_prof (HIP events around each launch, a run of its own) gives the generator's share.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaussian_processes_amd as gp                      # noqa: E402
from gaussian_processes_amd import _lib                  # noqa: E402

PROF = ["kmat", "gemm_trailing", "potrf_diag", "trsm_rows", "trsv", "mean", "reduce", "gemm_panel_bn64", "gemm_generic",
        "gemm_panel_bn128", "gemm_trailing_bn64", "transpose", "pred_grad", "extend", "randn"]


class Step(object):
    """A GPU step under its own time limit: the process exits (status 124) when the step overruns it."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        sys.stderr.write("[sample_bench] %s\n" % self.name)
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


def prof_read():
    lib, out = _lib.load(), {}
    for cls, name in enumerate(PROF):
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _lib.check(lib.gpx_prof_read(cls, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        if a.value:
            out[name] = {"launches": a.value, "ms": b.value, "work": c.value}
    return out


def one_m(g, xo, m, args):
    S, seed = args.size, 12345
    jitter = g._auto_jitter(xo)
    rng = np.random.RandomState(1)
    res = {"m": m, "size": S, "jitter": jitter, "cov_download_bytes": 8 * m * m, "sample_download_bytes": 8 * S * m}

    def device():
        t0 = time.perf_counter()
        f = g.sample(xo, size=S, seed=seed, jitter=jitter)
        return (time.perf_counter() - t0) * 1e3, f

    def host():
        t0 = time.perf_counter()
        C = g.cov(xo)
        t1 = time.perf_counter()
        C[np.diag_indices_from(C)] += jitter
        L = np.linalg.cholesky(C)
        t2 = time.perf_counter()
        f = g.mean(xo) + rng.standard_normal((S, m)) @ L.T
        t3 = time.perf_counter()
        return [(t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3], f

    with Step("warm-up and timing m = %d" % m, args.step_timeout):
        for _ in range(args.warmup):
            device()
            host()
        d_ms, h_ms = [], []
        for _ in range(args.repeats):
            d_ms.append(device()[0])
            h_ms.append(host()[0])
        res["device"] = stats(d_ms)
        res["host"] = stats([v[0] for v in h_ms])
        res["host_parts"] = {"cov_ms": stats([v[1] for v in h_ms]), "cholesky_ms": stats([v[2] for v in h_ms]),
                             "mean_product_ms": stats([v[3] for v in h_ms])}
        res["host_over_device"] = res["host"]["median_ms"] / res["device"]["median_ms"]
    with Step("gpx_prof split m = %d" % m, args.step_timeout):
        _lib.check(_lib.load().gpx_prof_enable(1))
        device()
        res["prof"] = prof_read()
        _lib.check(_lib.load().gpx_prof_enable(0))
        rn = res["prof"].get("randn")
        if rn:
            rn["bytes_per_s"] = rn["work"] / (rn["ms"] * 1e-3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--ms", default="1024,4096")
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=None, help="where the JSON goes besides stdout (default profiles/sample_bench_n<n>.json)")
    args = ap.parse_args()
    n, d = args.n, args.d
    ms = [int(v) for v in args.ms.split(",")]
    rng = np.random.RandomState(0)
    X = rng.uniform(-10, 10, (n, d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(n)
    Xo = np.random.RandomState(2).uniform(-10, 10, (max(ms), d))
    res = {"device": _lib.device_info(0)["name"], "n": n, "d": d, "dtype": "float64", "kernel": "gaussian", "s": 1.0,
           "repeats": args.repeats, "warmup": args.warmup,
           "clock": "host perf_counter around the synchronous calls, device and host route alternating; gpx_prof: HIP events "
                    "around each launch, in a run of its own", "ms": []}
    g = gp.GP(gp.GaussianKernel(1.0, 0.5 * np.sqrt(d)), X, y, s=1.0)
    with Step("fit n = %d" % n, args.step_timeout):
        t0 = time.perf_counter()
        res["log_lh"] = float(g.log_lh)
        res["first_fit_s"] = time.perf_counter() - t0
    for m in ms:
        res["ms"].append(one_m(g, np.ascontiguousarray(Xo[:m]), m, args))
    text = json.dumps(res)
    out = args.out or os.path.join(ROOT, "profiles", "sample_bench_n%d.json" % n)
    with open(out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
