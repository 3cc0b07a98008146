"""tools/sparse_bench.py -- time the sparse GP's fit and prediction ("Sparse GP on inducing points").

    python tools/sparse_bench.py [--n 1048576] [--d 32] [--m 1024,2048,4096] [--splits 0,1] [--predict 65536] [--repeats 3]
                                 [--chunk-cols 0] [--dtype float64] [--step-timeout 300]

One process, one JSON object per (M, split) on stdout; Gaussian kernel, synthetic inputs of oracle.synth_inputs.  `--splits`:
the depth slices per chunk of the Gram product, 0 = the library's plan, P >= 1 = exactly P (gpx_sgp_set_split): the plan
against one plain product per chunk is `--splits 0,1`.  Per (M, split): one warm-up fit, `repeats` fits whose
gpx_sgp_last_timing entries are reported as medians (HIP events on the handle's stream), then one fit under gpx_prof for the
Gram product's rate (GPX_PROF_SPARSE_GRAM: one pair of events around the products of each chunk; flops 2 c per element of
the lower triangle) and the kernel build's.  Prediction (mean and var at `--predict` points) is timed by a host clock around
the synchronous calls, once per M.  Every GPU step runs under a watchdog of its own (--step-timeout seconds): a step that
overruns it ends the process with exit status 124, so nothing further is started on the device.
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
from oracle import gp_oracle as orc                      # noqa: E402

STAGES = ("kuu", "build", "gram", "tail", "total")
FP64_MFMA_PEAK_TFLOPS = 78.6


class Step(object):
    """A GPU step under its own time limit: the process exits (status 124) when the step overruns it."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        sys.stderr.write("[sparse_bench] %s\n" % self.name)
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


def _refit(sg):
    sg._invalidate()
    elbo = sg.elbo
    return elbo, sg.fit_timing()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1048576)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--m", default="1024,2048,4096")
    ap.add_argument("--splits", default="0,1")
    ap.add_argument("--predict", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk-cols", type=int, default=0)
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--step-timeout", type=int, default=300)
    a = ap.parse_args()
    lib = _lib.load()
    X, y, Xo = orc.synth_inputs(a.n, a.d, a.predict)
    h, w, s = 1.0, 0.5 * np.sqrt(a.d), 1.0
    dtype_id = _lib.F64 if a.dtype == "float64" else _lib.F32
    for M in [int(v) for v in a.m.split(",")]:
        z = gp.SparseGP.subset_inducing(X, M, seed=3)
        sg = gp.SparseGP(gp.GaussianKernel(h, w), X, y, s, z, dtype=a.dtype, chunk_cols=a.chunk_cols)
        with Step("M = %d: upload" % M, a.step_timeout):
            st = sg._state()
        for split in [int(v) for v in a.splits.split(",")]:
            cols, chunks, slices, width = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)
            _lib.check(lib.gpx_debug_sgp_plan(dtype_id, a.n, M, a.chunk_cols, split, _lib.mem_free(), ctypes.byref(cols),
                                              ctypes.byref(chunks), ctypes.byref(slices), ctypes.byref(width)))
            _lib.check(lib.gpx_sgp_set_split(st.handle, split))
            with Step("M = %d split %d: warm-up fit" % (M, split), a.step_timeout):
                elbo, _ = _refit(sg)
            runs = []
            with Step("M = %d split %d: %d fits" % (M, split, a.repeats), a.step_timeout):
                for _ in range(a.repeats):
                    runs.append(_refit(sg)[1])
            with Step("M = %d split %d: one fit under gpx_prof" % (M, split), a.step_timeout):
                _lib.check(lib.gpx_prof_enable(1))
                _refit(sg)
                _, gram_ms, gram_flops = _prof(_lib.PROF_SPARSE_GRAM)
                _, kmat_ms, kmat_bytes = _prof(0)
                _lib.check(lib.gpx_prof_enable(0))
            rec = {"n": a.n, "d": a.d, "M": M, "dtype": a.dtype, "split_arg": split, "chunk_cols": cols.value, "chunks": chunks.value,
                   "slices": slices.value, "slice_cols": width.value, "elbo": float(elbo),
                   "fit_ms_median": {k: statistics.median(r[k] for r in runs) for k in STAGES},
                   "fit_ms_total_all": [r["total"] for r in runs],
                   "gram_ms_prof": gram_ms, "gram_tflops": gram_flops / gram_ms / 1e9 if gram_ms > 0 else None,
                   "kmat_ms_prof": kmat_ms, "kmat_gentries_per_s": kmat_bytes / (8 if a.dtype == "float64" else 4) / kmat_ms / 1e6 if kmat_ms > 0 else None}
            if rec["gram_tflops"] and a.dtype == "float64":
                rec["gram_fraction_of_fp64_mfma_peak"] = rec["gram_tflops"] / FP64_MFMA_PEAK_TFLOPS
            if split == 0 and a.predict > 0:
                with Step("M = %d: predict at %d points" % (M, a.predict), a.step_timeout):
                    sg.predict(Xo[:1024])                                    # warm-up
                    ts = []
                    for _ in range(a.repeats):
                        t0 = time.perf_counter()
                        sg.predict(Xo)
                        ts.append(1e3 * (time.perf_counter() - t0))
                rec["predict_m"] = a.predict
                rec["predict_ms_median"] = statistics.median(ts)
            print(json.dumps(rec))
            sys.stdout.flush()
        sg._dev.close()


if __name__ == "__main__":
    main()
