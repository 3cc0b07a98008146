"""tools/sparse_bench.py -- time the sparse GP's fit and prediction ("Sparse GP on inducing points").

    python tools/sparse_bench.py [--n 1048576] [--d 32] [--m 1024,2048,4096] [--splits 0,1] [--predict 65536] [--repeats 3]
                                 [--chunk-cols 0] [--dtype float64] [--step-timeout 300]

One process, one JSON object per (M, split) on stdout; Gaussian kernel, synthetic inputs of oracle.synth_inputs.  `--splits`:
the depth slices per chunk of the Gram product, 0 = the library's plan, P >= 1 = exactly P (gpx_sgp_set_split): the plan
against one plain product per chunk is `--splits 0,1`.  Per (M, split): one warm-up fit, `repeats` fits whose
gpx_sgp_last_timing entries are reported as medians (HIP events on the handle's stream), then one fit under gpx_prof for the
Gram product's rate (GPX_PROF_SPARSE_GRAM: one pair of events around the products of each chunk; flops 2 c per element of
the lower triangle) and the kernel build's.  With `--grad 1` (the default) the plan's row also carries the gradient of the
bound: gpx_sgp_last_grad_timing medians of `repeats` passes on the fit that is there (M x M part, builds, products K(x_c, z) T,
tile reductions, total), its ratio to the fit, the shares of the product and of the reduction, the product's TF/s
(2 M^2 N flops), the reduction's rate under gpx_prof (GPX_PROF_SPARSE_GRAD: kernel-derivative evaluations), one
`elbo_and_grad()` from new parameters by a host clock (what one optimize step costs) beside 2 (P + 1) fits (what central
differences would).  Beside it the JOINT pass (gpx_sgp_grad_z: the gradient in the inducing inputs from the same pass): the same
five stages with the z kernels' own two (gpx_sgp_last_zgrad_timing: Kuu's share, the chunks'), its ratio to the theta-only pass,
the z kernels' rate under gpx_prof (GPX_PROF_SPARSE_ZGRAD: kernel-derivative evaluations, c M per window of dimensions) beside
the reduction's on the same chunks, and one `elbo_and_grad(inducing=True)` after z moved (only z is uploaded).  Prediction (mean and var at `--predict` points) is timed by a host clock around
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
GRAD_STAGES = ("mm", "build", "product", "reduce", "total")
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


def _regrad(sg):
    """The gradient pass alone, on the fit that is there."""
    sg._memoized.pop("grad", None)
    grad = sg.delbo_dtheta
    return grad, sg.grad_timing()


def _rejoint(sg):
    """The joint pass alone, on the fit that is there: (grad_z, the five stages, the z kernels' two)."""
    sg._memoized.pop("grad", None)
    sg._memoized.pop("grad_z", None)
    grad_z = sg.delbo_dz
    return grad_z, sg.grad_timing(), sg.zgrad_timing()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grad", type=int, default=1)
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
            if split == 0 and a.grad:
                with Step("M = %d: warm-up gradient" % M, a.step_timeout):
                    _regrad(sg)
                gruns = []
                with Step("M = %d: %d gradients" % (M, a.repeats), a.step_timeout):
                    for _ in range(a.repeats):
                        gruns.append(_regrad(sg)[1])
                with Step("M = %d: one elbo_and_grad from new parameters (host clock)" % M, a.step_timeout):
                    t0 = time.perf_counter()
                    sg._invalidate()
                    sg.elbo_and_grad()
                    step_ms = 1e3 * (time.perf_counter() - t0)
                with Step("M = %d: one gradient under gpx_prof" % M, a.step_timeout):
                    _lib.check(lib.gpx_prof_enable(1))
                    grad, _ = _regrad(sg)
                    _, red_ms, red_evals = _prof(_lib.PROF_SPARSE_GRAD)
                    _lib.check(lib.gpx_prof_enable(0))
                fit_total = rec["fit_ms_median"]["total"]
                gmed = {k: statistics.median(r[k] for r in gruns) for k in GRAD_STAGES}
                nparams = len(sg.params)
                rec.update({"grad": [float(v) for v in grad], "grad_ms_median": gmed, "grad_ms_total_all": [r["total"] for r in gruns],
                            "grad_over_fit": gmed["total"] / fit_total if fit_total > 0 else None,
                            "grad_share_product": gmed["product"] / gmed["total"], "grad_share_reduce": gmed["reduce"] / gmed["total"],
                            "grad_product_tflops": 2.0 * M * M * a.n / gmed["product"] / 1e9 if gmed["product"] > 0 else None,
                            "grad_reduce_ms_prof": red_ms, "grad_reduce_gevals_per_s": red_evals / red_ms / 1e6 if red_ms > 0 else None,
                            "optimize_step_ms_host": step_ms, "finite_difference_step_ms": 2 * nparams * fit_total})   # nparams = P + 1: s is one
                with Step("M = %d: warm-up joint gradient" % M, a.step_timeout):
                    _rejoint(sg)
                jruns = []
                with Step("M = %d: %d joint gradients" % (M, a.repeats), a.step_timeout):
                    for _ in range(a.repeats):
                        jruns.append(_rejoint(sg)[1:])
                with Step("M = %d: one joint gradient under gpx_prof" % M, a.step_timeout):
                    _lib.check(lib.gpx_prof_enable(1))
                    grad_z = _rejoint(sg)[0]
                    _, jred_ms, jred_evals = _prof(_lib.PROF_SPARSE_GRAD)
                    zl, z_ms, z_evals = _prof(_lib.PROF_SPARSE_ZGRAD)
                    _lib.check(lib.gpx_prof_enable(0))
                with Step("M = %d: one joint elbo_and_grad after z moved (host clock)" % M, a.step_timeout):
                    t0 = time.perf_counter()
                    sg.z = np.array(sg.z) + 1e-3
                    sg.elbo_and_grad(inducing=True)
                    jstep_ms = 1e3 * (time.perf_counter() - t0)
                    sg.z = z
                jmed = {k: statistics.median(r[0][k] for r in jruns) for k in GRAD_STAGES}
                zmed = {k: statistics.median(r[1][k] for r in jruns) for k in ("kuu", "chunks")}
                rec.update({"joint_ms_median": jmed, "joint_zgrad_ms_median": zmed, "joint_ms_total_all": [r[0]["total"] for r in jruns],
                            "joint_over_theta": jmed["total"] / gmed["total"] if gmed["total"] > 0 else None,
                            "grad_z_absmax": float(np.abs(grad_z).max()), "zgrad_launches_prof": zl, "zgrad_ms_prof": z_ms,
                            "zgrad_gevals_per_s": z_evals / z_ms / 1e6 if z_ms > 0 else None,
                            "joint_reduce_gevals_per_s": jred_evals / jred_ms / 1e6 if jred_ms > 0 else None,
                            "joint_optimize_step_ms_host": jstep_ms})
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
