"""tools/var_bench.py -- time GP.var against GP.cov at the headline size (profiles/var_n65536.json).

    python tools/var_bench.py [--n 65536] [--d 32] [--repeats 5] [--step-timeout 300] [--skip-caps]
    python tools/var_bench.py --kernel-only [--rows 4096] [--n 65536]      # gpx_d_var_rows alone (for a kernel trace)

One process, one JSON object on stdout.  Every GPU step runs under a watchdog of its own (--step-timeout seconds): a step
that overruns it ends the process with exit status 124, so nothing further is started on the device.  Times are a host
clock around calls that end in a download (they synchronise); the kernel-only mode uses events on the null stream.

  (a) cov(xo) and var(xo) at m = 1000 and m = 4096, alternating in the same run
  (b) var at m = n with the automatic chunking: ms, chunks, n^2 m flop over the time against the fp64 MFMA peak --
      the TRSM's whole-call rate, not a kernel figure
  (c) --kernel-only: bytes over time of the finishing kernel on one chunk against the HBM peak
  (d) the chunk size at 1024 / 2048 / 4096 / 8192 rows at m = n
"""
import argparse
import ctypes
import faulthandler
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_processes_amd as gp                      # noqa: E402
from gaussian_processes_amd import _lib                  # noqa: E402

FP64_MFMA_PEAK_TFLOPS = 78.6                             # MI355X, dense fp64 matrix
HBM_PEAK_TBPS = 8.0                                      # MI355X HBM3E


class Step(object):
    """A GPU step under its own time limit: the process exits (status 124) when the step overruns it."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        sys.stderr.write("[var_bench] %s\n" % self.name)
        sys.stderr.flush()
        faulthandler.dump_traceback_later(self.seconds, exit=False, file=sys.stderr)
        self._t = _watchdog(self.seconds)
        return self

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()
        self._t.cancel()
        return False


def _watchdog(seconds):
    import threading
    t = threading.Timer(seconds + 1.0, lambda: os._exit(124))
    t.daemon = True
    t.start()
    return t


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "spread_ms": max(ms) - min(ms), "runs_ms": [round(v, 3) for v in ms]}


def timed(f, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def kernel_only(args):
    lib = _lib.load()
    rows, n = args.rows, args.n
    ldx = (n + 15) // 16 * 16
    res = {"mode": "kernel-only", "rows": rows, "n": n, "ldx": ldx, "device": _lib.device_info(0)["name"], "by_dtype": {}}
    for name, dtype, es in (("float64", _lib.F64, 8), ("float32", _lib.F32, 4)):
        with Step("gpx_d_var_rows %s" % name, args.step_timeout):
            X, kd, out = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            _lib.check(lib.gpx_malloc(ctypes.byref(X), rows * ldx * es))
            _lib.check(lib.gpx_malloc(ctypes.byref(kd), rows * 8))
            _lib.check(lib.gpx_malloc(ctypes.byref(out), rows * 8))
            ev = [ctypes.c_void_p() for _ in range(2)]
            for e in ev:
                _lib.check(lib.gpx_event_create(ctypes.byref(e)))
            try:
                _lib.check(lib.gpx_memset(X, 0, rows * ldx * es, None))
                _lib.check(lib.gpx_memset(kd, 0, rows * 8, None))
                ms = []
                for i in range(args.warmup + args.repeats):
                    _lib.check(lib.gpx_event_record(ev[0], None))
                    _lib.check(lib.gpx_d_var_rows(dtype, _lib.KERNEL_GAUSSIAN, X, rows, n, ldx, None, 0, None, kd, out, None))
                    _lib.check(lib.gpx_event_record(ev[1], None))
                    _lib.check(lib.gpx_event_sync(ev[1]))
                    t = ctypes.c_float(0)
                    _lib.check(lib.gpx_event_elapsed_ms(ev[0], ev[1], ctypes.byref(t)))
                    if i >= args.warmup:
                        ms.append(t.value)
                nbytes = rows * n * es
                r = stats(ms)
                r["bytes"] = nbytes
                r["TBps"] = nbytes / (r["median_ms"] * 1e-3) / 1e12
                r["share_of_hbm_peak"] = r["TBps"] / HBM_PEAK_TBPS
                res["by_dtype"][name] = r
            finally:
                for e in ev:
                    lib.gpx_event_destroy(e)
                for b in (X, kd, out):
                    lib.gpx_free(b)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--skip-caps", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--rows", type=int, default=4096)
    args = ap.parse_args()
    if args.kernel_only:
        print(json.dumps(kernel_only(args)))
        return
    N, d = args.n, args.d
    rng = np.random.RandomState(0)
    X = rng.uniform(-10, 10, (N, d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(N)
    Xo = np.random.RandomState(1).uniform(-10, 10, (N, d))
    res = {"n": N, "d": d, "dtype": "float64", "s": 1.0, "repeats": args.repeats, "device": _lib.device_info(0)["name"],
           "clock": "host perf_counter around calls that end in a download"}
    g = gp.GP(gp.GaussianKernel(1.0, 0.5 * np.sqrt(d)), X, y, s=1.0)
    with Step("fit", args.step_timeout):
        t0 = time.perf_counter()
        res["log_lh"] = float(g.log_lh)
        res["fit_s"] = time.perf_counter() - t0
    res["cov_vs_var"] = {}
    for m in (1000, 4096):
        if m > N:
            continue
        xo = Xo[:m]
        with Step("cov / var at m = %d" % m, args.step_timeout):
            for _ in range(args.warmup):
                g.cov(xo), g.var(xo)
            cov_ms, var_ms = [], []
            for _ in range(args.repeats):            # alternating: both see the same state of the machine
                cov_ms += timed(lambda: g.cov(xo), 1)
                var_ms += timed(lambda: g.var(xo), 1)
            res["cov_vs_var"][str(m)] = {"cov": stats(cov_ms), "var": stats(var_ms),
                                         "chunks": _lib.var_plan(_lib.F64, N, m)[1]}
    with Step("var at m = n, automatic chunking", args.step_timeout):
        g.var(Xo)
        ms = timed(lambda: g.var(Xo), args.repeats)
        rows, chunks, nbytes = _lib.var_plan(_lib.F64, N, N)
        r = stats(ms)
        r.update(m=N, rows_per_chunk=rows, chunks=chunks, bytes_per_chunk=nbytes)
        r["trsm_flop"] = float(N) * N * N
        r["whole_call_TFLOPs"] = r["trsm_flop"] / (r["median_ms"] * 1e-3) / 1e12
        r["whole_call_share_of_fp64_mfma_peak"] = r["whole_call_TFLOPs"] / FP64_MFMA_PEAK_TFLOPS
        res["var_m_eq_n"] = r
    if not args.skip_caps:
        res["chunk_rows_sweep"] = {}
        for rows in (1024, 2048, 4096, 8192):
            with Step("var at m = n, chunk_rows = %d" % rows, args.step_timeout):
                g.var(Xo[:2 * rows], chunk_rows=rows)          # (the solve's staging block grows here, not in the timing)
                res["chunk_rows_sweep"][str(rows)] = stats(timed(lambda: g.var(Xo, chunk_rows=rows), args.repeats))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
