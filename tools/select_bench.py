"""tools/select_bench.py -- time the greedy selection of inducing points ("Selecting inducing points").

    python tools/select_bench.py [--n 1048576] [--d 32] [--m 1024,2048] [--dtypes float64,float32] [--elbo 1] [--step-timeout 300]

One process, one JSON object per (M, dtype) on stdout; Gaussian kernel, synthetic inputs of oracle.synth_inputs (the settings of
tools/sparse_bench.py).  Per (M, dtype): one small warm-up call, then ONE SparseGP.greedy_inducing under gpx_prof: the wall
time of the call by a host clock (upload of x included), the device time of all its launches (GPX_PROF_SELECT: one pair of events
around them) and the bytes of R they moved per second (sizeof(T) n count (count + 1) / 2 over that time), the rate of the steps
m >= 256 alone from the difference to a second call with M = 256 (each step reads every row before it), and -- with `--elbo 1`
-- the bound of a fit at the greedy z beside the bound at SparseGP.subset_inducing's z (seed 3) for the same M.  Every GPU
step runs under a watchdog of its own (--step-timeout seconds): a step that overruns it ends the process with exit status
124, so nothing further is started on the device.
"""
import argparse
import ctypes
import faulthandler
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_processes_amd as gp                      # noqa: E402
from gaussian_processes_amd import _lib                  # noqa: E402
from oracle import gp_oracle as orc                      # noqa: E402


class Step(object):
    """A GPU step under its own time limit: the process exits (status 124) when the step overruns it."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        sys.stderr.write("[select_bench] %s\n" % self.name)
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


def _prof(cls):
    launches, ms, work = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    _lib.check(_lib.load().gpx_prof_read(cls, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(work)))
    return launches.value, ms.value, work.value


def _select(K, X, M, dtype):
    """(z, info, wall ms, device ms, bytes of R) of one call under gpx_prof."""
    lib = _lib.load()
    _lib.check(lib.gpx_prof_enable(1))
    t0 = time.perf_counter()
    z, info = gp.SparseGP.greedy_inducing(K, X, M, dtype=dtype, return_info=True)
    wall = 1e3 * (time.perf_counter() - t0)
    _, ms, work = _prof(_lib.PROF_SELECT)
    _lib.check(lib.gpx_prof_enable(0))
    return z, info, wall, ms, work


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1048576)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--m", default="1024,2048")
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--elbo", type=int, default=1)
    ap.add_argument("--head", type=int, default=256)
    ap.add_argument("--step-timeout", type=int, default=300)
    a = ap.parse_args()
    X, y, _ = orc.synth_inputs(a.n, a.d, 1)
    h, w, s = 1.0, 0.5 * np.sqrt(a.d), 1.0
    K = gp.GaussianKernel(h, w)
    for dtype in a.dtypes.split(","):
        es = 8 if dtype == "float64" else 4
        with Step("%s: warm-up" % dtype, a.step_timeout):
            gp.SparseGP.greedy_inducing(K, X[:4096], 16, dtype=dtype)
        head = None
        if a.head > 0:
            with Step("%s: M = %d (the head, for the rate of the later steps)" % (dtype, a.head), a.step_timeout):
                head = _select(K, X, a.head, dtype)
        for M in [int(v) for v in a.m.split(",")]:
            with Step("%s: M = %d" % (dtype, M), a.step_timeout):
                z, info, wall, ms, work = _select(K, X, M, dtype)
            k0 = float(K.diag(X[:1])[0])
            rec = {"n": a.n, "d": a.d, "M": M, "dtype": dtype, "count": info["count"], "tol": info["tol"], "wall_ms": wall, "select_ms": ms,
                   "R_bytes_moved": work, "R_tbytes_per_s": work / ms / 1e9 if ms > 0 else None,
                   "R_bytes_expected": es * a.n * info["count"] * (info["count"] + 1) / 2.0,
                   "us_per_step": 1e3 * ms / max(info["count"], 1),
                   "last_pivot_over_k0": float(info["pivot"][-1] / k0), "trace_over_kff": float(info["trace"][-1] / info["trace"][0])}
            if head is not None and info["count"] > head[1]["count"] == a.head and ms > head[3]:
                rec["tail_from_step"] = a.head
                rec["tail_ms"] = ms - head[3]
                rec["tail_R_tbytes_per_s"] = (work - head[4]) / (ms - head[3]) / 1e9
            if a.elbo:
                with Step("%s: M = %d: the bound at the greedy z and at a random subset" % (dtype, M), a.step_timeout):
                    sg = gp.SparseGP(K, X, y, s, z, dtype=dtype)
                    rec["elbo_greedy"] = float(sg.elbo)
                    sg.z = gp.SparseGP.subset_inducing(X, info["count"], seed=3)
                    rec["elbo_subset"] = float(sg.elbo)
                    sg._dev.close()
            print(json.dumps(rec))
            sys.stdout.flush()


if __name__ == "__main__":
    main()
