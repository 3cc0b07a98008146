"""tools/cg_bench.py -- time the iterative exact GP ("Exact GP past the factor: preconditioned CG").

    python tools/cg_bench.py [--sweep 65536] [--ranks 0,32,128,512] [--large 262144] [--predict 65536] [--read 8192,65536]
                             [--d 32] [--dense 1] [--lh 65536,262144] [--probes 32] [--step-timeout 300]

One process, one JSON object per measurement on stdout; Gaussian kernel (h = 1, w = sqrt(d) / 2, s = 1), synthetic inputs of
oracle.synth_inputs -- the benchmark's data.  Four measurements, each skipped with 0 (--lh: with an empty list, its default):
  --sweep N    IterativeGP.inv_Kxx_y at N for every rank of --ranks: iterations to tol, gpx_cg_last_timing (the preconditioner's
               build; of the solve: products, preconditioner applies, vector kernels, status reads, total), milliseconds per
               iteration, build + solve, a host clock around the whole call, device bytes; beside it the dense gp.GP fit at the
               same N (--dense 1) by a host clock, and the cost model's time for one product: n^2 (2 d + 40) fp64 vector flops.
  --large N    one solve with the default rank at an N the dense GP cannot hold, one mean at --predict points, the handle's device
               bytes and the drop in free device memory; gp.GP's refusal at the same N is the comparison.
  --read LIST  the per-iteration status read's share of an iteration at each N: rank 0, maxiter 20 and a tolerance of 1e-300, so
               that the solve runs on to 20 iterations or to a residual of exactly 0.
  --lh LIST    the marginal-likelihood pass at each N, default rank, for every probe count of --probes: the solve for y first (its
               iterations and time), then one IterativeGP.log_lh_estimate and one log_lh_and_grad (a fresh pass each: the memo is
               dropped) by a host clock, with the probes' iteration counts, the estimate's standard error, and from the live
               profile the launches and milliseconds of the low-rank tile reduction (GPX_PROF_LOWRANK) next to its flop model
               n^2 (d + T) FMAs per launch.
Every GPU step runs under a watchdog of its own (--step-timeout seconds): a step that overruns it ends the process with exit
status 124, so nothing further is started on the device.
"""
import argparse
import faulthandler
import json
import os
import sys
import threading
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_processes_amd as gp                      # noqa: E402
from gaussian_processes_amd import _lib                  # noqa: E402
from oracle import gp_oracle as orc                      # noqa: E402

FP64_VECTOR_PEAK_TFLOPS = 78.6


class Step(object):
    """A GPU step under its own time limit: the process exits (status 124) when the step overruns it."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        sys.stderr.write("[cg_bench] %s\n" % self.name)
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


def model_ms(n, d):
    """The cost model's time of one product with K: n^2 (2 d + 40) fp64 vector flops at the vector peak."""
    return float(n) * n * (2 * d + 40) / (FP64_VECTOR_PEAK_TFLOPS * 1e12) * 1e3


def emit(rec):
    print(json.dumps(rec))
    sys.stdout.flush()


def solve_record(g, n, d):
    """One inv_Kxx_y from scratch on the data that is on the device: the timing split, iterations and a host clock."""
    g._invalidate()
    g._state().pre_key = None                                # (the preconditioner is built again: its time belongs to the total)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        t0 = time.perf_counter()
        g.inv_Kxx_y
        host_ms = 1e3 * (time.perf_counter() - t0)
    info, t = g.solve_info, g.timing()
    its = max(1, abs(int(info["iterations"][0])))
    return {"n": n, "d": d, "rank_asked": g.precond_rank, "rank": int(info["rank"]), "iterations": int(info["iterations"][0]),
            "converged": bool(info["converged"][0]), "relres": float(info["relres"][0]), "tol": g.tol, "maxiter": g.maxiter,
            "ms": t, "ms_per_iteration": {k: t[k] / its for k in ("product", "apply", "vector", "read", "total")},
            "build_plus_solve_ms": t["precond"] + t["total"], "host_ms": host_ms, "read_share_of_solve": t["read"] / t["total"] if t["total"] > 0 else None,
            "model_product_ms": model_ms(n, d), "device_bytes": g.device_bytes}


def prof_lowrank():
    """(launches, milliseconds) of the low-rank tile reduction since the profile was enabled."""
    import ctypes
    a, b, c = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    _lib.check(_lib.load().gpx_prof_read(_lib.PROF_LOWRANK, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return int(a.value), b.value


def lh_record(g, n, d, probes):
    """One estimate and one estimate with gradient, each a fresh pass, after the solve for y."""
    lib = _lib.load()
    rec = {"measurement": "lh", "n": n, "d": d, "probes": probes, "rank": int(g.solve_info["rank"]),
           "y_iterations": int(g.solve_info["iterations"][0])}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for name, call in (("estimate", lambda: g.log_lh_estimate(probes=probes, return_info=True)),
                           ("gradient", lambda: g.log_lh_and_grad(probes=probes))):
            for key in [k for k in g._memoized if isinstance(k, tuple) and k[0] == "lh"]:
                del g._memoized[key]
            _lib.check(lib.gpx_prof_enable(1))
            t0 = time.perf_counter()
            out = call()
            rec[name + "_host_ms"] = 1e3 * (time.perf_counter() - t0)
            launches, ms = prof_lowrank()
            _lib.check(lib.gpx_prof_enable(0))
            rec[name + "_total_ms"] = g.timing()["total"]
            if name == "estimate":
                info = out[1]
                rec.update(value=float(out[0]), stderr=info["stderr"], probe_iterations_max=int(np.abs(info["iterations"]).max()),
                           probe_iterations_mean=float(np.abs(info["iterations"]).mean()), converged=bool(info["converged"].all()))
            else:
                rec.update(reduce_launches=launches, reduce_ms=ms, grad=[float(v) for v in out[1]],
                           reduce_model_ms=(float(n) * n * 2 * (d + min(probes, 32)) * (launches - 1) + float(n) * n * 2 * (d + 1))
                           / (FP64_VECTOR_PEAK_TFLOPS * 1e12) * 1e3)
    rec["device_bytes"] = g.device_bytes
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", type=int, default=65536)
    ap.add_argument("--ranks", default="0,32,128,512")
    ap.add_argument("--large", type=int, default=262144)
    ap.add_argument("--predict", type=int, default=65536)
    ap.add_argument("--read", default="8192,65536")
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--dense", type=int, default=1)
    ap.add_argument("--lh", default="")
    ap.add_argument("--probes", default="32")
    ap.add_argument("--step-timeout", type=int, default=300)
    a = ap.parse_args()
    _lib.load()
    d = a.d
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    if a.sweep > 0:
        n = a.sweep
        X, y, _ = orc.synth_inputs(n, d, 1)
        g = gp.IterativeGP(gp.GaussianKernel(h, w), X, y, s, precond_rank=0)
        with Step("sweep N = %d: upload and warm-up" % n, a.step_timeout):
            g.maxiter = 2
            solve_record(g, n, d)
            g.maxiter = None
        for rank in [int(v) for v in a.ranks.split(",")]:
            g.precond_rank = rank
            with Step("sweep N = %d rank %d" % (n, rank), a.step_timeout):
                rec = solve_record(g, n, d)
            rec["measurement"] = "sweep"
            emit(rec)
        g._dev.close()
        del g
        if a.dense:
            with Step("dense fit N = %d" % n, a.step_timeout):
                dense = gp.GP(gp.GaussianKernel(h, w), X, y, s)
                t0 = time.perf_counter()
                dense.inv_Kxx_y
                emit({"measurement": "dense", "n": n, "d": d, "host_ms": 1e3 * (time.perf_counter() - t0)})
            del dense
    if a.large > 0:
        n = a.large
        X, y, Xo = orc.synth_inputs(n, d, a.predict)
        free0 = _lib.mem_free()
        g = gp.IterativeGP(gp.GaussianKernel(h, w), X, y, s)
        with Step("large N = %d: one solve, default rank" % n, a.step_timeout):
            g._state()
            rec = solve_record(g, n, d)
        with Step("large N = %d: mean at %d points" % (n, a.predict), a.step_timeout):
            t0 = time.perf_counter()
            mean = g.mean(Xo)
            rec["mean_m"], rec["mean_host_ms"] = a.predict, 1e3 * (time.perf_counter() - t0)
            rec["mean_finite"] = bool(np.all(np.isfinite(mean)))
        rec["free_memory_drop_bytes"] = free0 - _lib.mem_free()
        rec["factor_bytes"] = 8 * n * n
        try:
            gp.GP(gp.GaussianKernel(h, w), X, y, s).inv_Kxx_y
            rec["dense_refusal"] = None
        except Exception as exc:          # the refusal IS the comparison
            rec["dense_refusal"] = "%s: %s" % (type(exc).__name__, str(exc)[:300])
        rec["measurement"] = "large"
        emit(rec)
        g._dev.close()
    for n in [int(v) for v in a.read.split(",") if v]:
        X, y, _ = orc.synth_inputs(n, d, 1)
        g = gp.IterativeGP(gp.GaussianKernel(h, w), X, y, s, precond_rank=0, tol=1e-300, maxiter=20)
        with Step("status read N = %d: 20 iterations, twice" % n, a.step_timeout):
            solve_record(g, n, d)
            rec = solve_record(g, n, d)
        rec["measurement"] = "read"
        emit(rec)
        g._dev.close()
    for n in [int(v) for v in a.lh.split(",") if v]:
        X, y, _ = orc.synth_inputs(n, d, 1)
        g = gp.IterativeGP(gp.GaussianKernel(h, w), X, y, s)
        with Step("lh N = %d: the solve for y" % n, a.step_timeout):
            g.inv_Kxx_y
        for probes in [int(v) for v in a.probes.split(",")]:
            with Step("lh N = %d, %d probes" % (n, probes), a.step_timeout):
                emit(lh_record(g, n, d, probes))
        g._dev.close()


if __name__ == "__main__":
    main()
