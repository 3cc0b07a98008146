"""tools/mg_cov_bench.py [--n 32768 65536] [--d 32] [--m 1000] [--nb ...] [--reps 3] -- the posterior covariance of the
multi-GPU handle on ONE RCCL rank (gpx_mg_cov: L stays in the block-cyclic layout, one all-reduce per block column)
against the single-GPU gpx_gp_cov on the same data, fp64.  Prints one JSON line per (N, nb): median ms of each, the
ratio, the fraction of the fp64 MFMA peak by the (n^2 m + n m^2) flop of the two triangular products, and the largest
difference between the two results.  The world-1 handle is timed as a user gets it (no collective is issued) and with
GPX_FORCE_COLLECTIVES=1 (every block's all-reduce a real RCCL call)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_processes_amd as gp  # noqa: E402
from gaussian_processes_amd import multi_gpu  # noqa: E402
from oracle import gp_oracle as orc  # noqa: E402

PEAK_F64 = 78.6e12            # MI355X fp64 matrix-core peak, flop/s


def median_ms(f, reps):
    f()                                           # warm: scratch buffers, operator route
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()                                 # synchronous: returns with the result on the host
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[32768, 65536])
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--nb", type=int, nargs="*", default=None, help="block widths (default: multi_gpu.default_nb)")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    d, m = a.d, a.m
    for N in a.n:
        X, y, Xo = orc.synth_inputs(N, d, m)
        h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
        params = np.array([h, w])
        g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s)
        g.log_lh
        gp_ms, ref = median_ms(lambda: g.cov(Xo), a.reps)
        del g
        flop = float(N) * N * m + float(N) * m * m
        for nb in (a.nb or [multi_gpu.default_nb(N, 1)]):
            mg = multi_gpu.NativeDistributedGP(N, d, nb=nb, backend="rccl", device=0)
            try:
                mg.set_data(X, y)
                mg.fit(params, s)
                mg_ms, out = median_ms(lambda: mg.cov(params, Xo), a.reps)
                os.environ["GPX_FORCE_COLLECTIVES"] = "1"
                try:
                    forced_ms, out_f = median_ms(lambda: mg.cov(params, Xo), a.reps)
                finally:
                    del os.environ["GPX_FORCE_COLLECTIVES"]
            finally:
                mg.close()
            scale = float(np.abs(ref).max())
            print(json.dumps({
                "N": N, "d": d, "m": m, "nb": nb, "gp_cov_ms": round(gp_ms, 2), "mg_cov_ms": round(mg_ms, 2),
                "mg_cov_forced_collectives_ms": round(forced_ms, 2), "ratio_mg_over_gp": round(mg_ms / gp_ms, 3),
                "floor_ms": round(flop / PEAK_F64 * 1e3, 1), "peak_frac_gp": round(flop / (gp_ms * 1e-3) / PEAK_F64, 3),
                "peak_frac_mg": round(flop / (mg_ms * 1e-3) / PEAK_F64, 3),
                "max_rel_diff": float(np.abs(out - ref).max() / scale), "forced_equal": bool(np.array_equal(out, out_f)),
                "device": gp._lib.device_info(0)["name"]}), flush=True)


if __name__ == "__main__":
    main()
