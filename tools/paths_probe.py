"""tools/paths_probe.py -- the measurements behind GPX_KAPPLY_FUSED_MAX and DESIGN.md, "Posterior paths".

    python tools/paths_probe.py [apply] [--shapes 65536x32,8192x3] [--m 4096] [--S 1,4,8,16,32,64,128] [--dtypes float64,float32]
                                [--repeats 5] [--create 65536x32] [--size 64] [--features 1024] [--step-timeout 300] [--out FILE]
    python tools/paths_probe.py grad [--shapes ...] [--m 4096] [--S 1,4,8,16,32,64] [--dtypes ...] [--repeats 5] [--size 8]
                                [--features 1024] [--step-timeout 300] [--out FILE]

One process, one JSON object on stdout (and in --out).  Mode `apply` (the default), three measurements:

  crossover  gpx_d_kmat_apply on both of its routes -- forced through GPX_KAPPLY_FUSED_MAX and asserted on the route counters
             -- at every (n x d, dtype, S): out (S x m) += K(xo, x) V^T on random points, the two routes ALTERNATING.
             `fused_max`: per dtype, the largest measured S at which the fused route is not slower in ANY shape -- the
             two defaults in csrc/gpx_tune.h.
  mean       the fused route at S = 1 against gpx_d_mean on the same (m, n, d): the same pairs, one more FMA and one
             accumulate pass.
  create     (--create n x d; needs a fit of n points) GP.sample_paths(size, features) at that size, fp64: the stage times
             of gpx_debug_paths_timing, the host clock around the call, and one evaluation at m points.

Mode `grad`, the measurements of DESIGN "Posterior paths", "The gradient of a path":

  primitive  gpx_d_kmat_apply_grad at every (n x d, dtype, S), beside the fused gpx_d_kmat_apply at the same S (forced through
             GPX_KAPPLY_FUSED_MAX) and, at S = 1, gpx_d_pred_grad on the same points -- the three ALTERNATING.  `per_eval`: the
             time per kernel evaluation (m n per group of vectors [and window of dimensions]) of the gradient over that of
             the apply; `over_W_applies`: the gradient's time over W = cdiv(d, DP) fused applies.
  paths      (needs a fit of n points per shape and dtype) PosteriorPaths.value_and_grad(xo) at --size paths on the host
             clock, upload and download included, against 2 d + 1 calls of paths(xo) -- central differences, the only route
             without the gradient; the best of three each.

Device times are HIP events on the null stream around `repeats` back-to-back calls, after one warm-up call of the same
shape.  Every GPU step runs under a watchdog of its own (--step-timeout seconds): a step that overruns it ends the process
with exit status 124, so nothing further is started on the device."""
import argparse
import ctypes
import faulthandler
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaussian_processes_amd as gp                      # noqa: E402
from gaussian_processes_amd import _lib                  # noqa: E402

_NP = {"float64": np.float64, "float32": np.float32}
_ID = {"float64": _lib.F64, "float32": _lib.F32}


class Step(object):
    """A GPU step under its own time limit: the process exits (status 124) when the step overruns it."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def __enter__(self):
        sys.stderr.write("[paths_probe] %s\n" % self.name)
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


class Device(object):
    """gpx_malloc'ed blocks and one pair of events."""

    def __init__(self):
        self.lib, self.bufs = _lib.load(), []
        self.e0, self.e1 = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(self.lib.gpx_event_create(ctypes.byref(self.e0)))
        _lib.check(self.lib.gpx_event_create(ctypes.byref(self.e1)))

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        b = ctypes.c_void_p()
        _lib.check(self.lib.gpx_malloc(ctypes.byref(b), max(arr.nbytes, 16)))
        self.bufs.append(b)
        _lib.check(self.lib.gpx_memcpy_h2d(b, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes, None))
        return b

    def free_all(self):
        _lib.check(self.lib.gpx_device_sync())
        for b in self.bufs:
            self.lib.gpx_free(b)
        self.bufs = []

    def time_ms(self, call, repeats):
        """Milliseconds per call: one warm-up, then `repeats` calls between two events."""
        call()
        _lib.check(self.lib.gpx_device_sync())
        _lib.check(self.lib.gpx_event_record(self.e0, None))
        for _ in range(repeats):
            call()
        _lib.check(self.lib.gpx_event_record(self.e1, None))
        _lib.check(self.lib.gpx_event_sync(self.e1))
        ms = ctypes.c_float(0)
        _lib.check(self.lib.gpx_event_elapsed_ms(self.e0, self.e1, ctypes.byref(ms)))
        return ms.value / repeats


def shape_probe(dev, n, d, m, Ss, dtype, args):
    T, rng, lib = _NP[dtype], np.random.RandomState(n + d), dev.lib
    prm = np.array([1.0, 0.5 * np.sqrt(d)])
    Smax = max(Ss)
    ldv, ldo = (n + 15) // 16 * 16, (m + 15) // 16 * 16
    dx, dxo = dev.put(rng.uniform(-10, 10, (n, d)).astype(T)), dev.put(rng.uniform(-10, 10, (m, d)).astype(T))
    dV, dout = dev.put(rng.randn(Smax, ldv).astype(T)), dev.put(np.zeros((Smax, ldo), dtype=T))
    res = {"n": n, "d": d, "m": m, "dtype": dtype, "S": []}

    def apply(S):
        _lib.check(lib.gpx_d_kmat_apply(_ID[dtype], _lib.KERNEL_GAUSSIAN, dxo, m, dx, n, d, _lib.dptr(prm), dV, ldv, S, dout, ldo, None))

    def routed(S, fused):
        _lib.kapply_fused_max(1 << 20 if fused else 0)
        _lib.route_reset()
        ms = dev.time_ms(lambda: apply(S), args.repeats)
        hit, other = ((_lib.ROUTE_KAPPLY_FUSED, _lib.ROUTE_KAPPLY_GEMM) if fused else (_lib.ROUTE_KAPPLY_GEMM, _lib.ROUTE_KAPPLY_FUSED))
        assert _lib.route_count(hit) > 0 and _lib.route_count(other) == 0
        return ms

    for S in Ss:
        with Step("kmat_apply n=%d d=%d %s S=%d" % (n, d, dtype, S), args.step_timeout):
            f1, g1 = routed(S, True), routed(S, False)
            f2, g2 = routed(S, True), routed(S, False)
            res["S"].append({"S": S, "fused_ms": min(f1, f2), "gemm_ms": min(g1, g2), "runs_ms": [f1, g1, f2, g2]})
    _lib.kapply_fused_max(-1)
    with Step("fused S=1 against gpx_d_mean n=%d d=%d %s" % (n, d, dtype), args.step_timeout):
        dmean = dev.put(np.zeros(m, dtype=T))

        def mean():
            _lib.check(lib.gpx_d_mean(_ID[dtype], _lib.KERNEL_GAUSSIAN, dxo, m, dx, n, d, _lib.dptr(prm), dV, dmean, None))
        _lib.kapply_fused_max(1 << 20)
        a1, m1 = dev.time_ms(lambda: apply(1), args.repeats), dev.time_ms(mean, args.repeats)
        a2, m2 = dev.time_ms(lambda: apply(1), args.repeats), dev.time_ms(mean, args.repeats)
        _lib.kapply_fused_max(-1)
        res["mean"] = {"fused_S1_ms": min(a1, a2), "mean_ms": min(m1, m2), "ratio": min(a1, a2) / min(m1, m2), "runs_ms": [a1, m1, a2, m2]}
    dev.free_all()
    return res


def kgrad_block(S, d):
    """(points, vectors, dimensions) of gpx_d_kmat_apply_grad's register block: kapply_grad_shape in csrc/gpx_stream.hip."""
    if d <= 4:
        return (4, 1, 4) if S == 1 else (4, 2, 4) if S == 2 else (2, 4, 4)
    return (1, 1, 16) if S == 1 else (1, 2, 16) if S == 2 else (1, 4, 8)


def kapply_block(S):
    """(points, vectors) of the fused gpx_d_kmat_apply: kapply_shape in csrc/gpx_stream.hip."""
    return (8, 1) if S == 1 else (8, 4) if S <= 4 else (4, 8)


def grad_shape_probe(dev, n, d, m, Ss, dtype, args):
    T, rng, lib = _NP[dtype], np.random.RandomState(n + d), dev.lib
    prm = np.array([1.0, 0.5 * np.sqrt(d)])
    Smax = max(Ss)
    ldv, ldo = (n + 15) // 16 * 16, (m + 15) // 16 * 16
    dx, dxo = dev.put(rng.uniform(-10, 10, (n, d)).astype(T)), dev.put(rng.uniform(-10, 10, (m, d)).astype(T))
    dV, dout = dev.put(rng.randn(Smax, ldv).astype(T)), dev.put(np.zeros((Smax, ldo), dtype=T))
    dgrad, dpg = dev.put(np.zeros((Smax, m * d), dtype=T)), dev.put(np.zeros((m, d)))
    res = {"n": n, "d": d, "m": m, "dtype": dtype, "S": []}

    def grad(S):
        _lib.check(lib.gpx_d_kmat_apply_grad(_ID[dtype], _lib.KERNEL_GAUSSIAN, dxo, m, dx, n, d, _lib.dptr(prm), None, dV, ldv, S, dgrad,
                                             m * d, None))

    def apply(S):
        _lib.check(lib.gpx_d_kmat_apply(_ID[dtype], _lib.KERNEL_GAUSSIAN, dxo, m, dx, n, d, _lib.dptr(prm), dV, ldv, S, dout, ldo, None))

    def pred_grad():
        _lib.check(lib.gpx_d_pred_grad(_ID[dtype], _lib.KERNEL_GAUSSIAN, dxo, m, dx, n, d, _lib.dptr(prm), dV, None, 0, 1.0, dpg, None))

    _lib.kapply_fused_max(1 << 20)
    for S in Ss:
        with Step("kmat_apply_grad n=%d d=%d %s S=%d" % (n, d, dtype, S), args.step_timeout):
            calls = [lambda: grad(S), lambda: apply(S)] + ([pred_grad] if S == 1 else [])
            runs = [[dev.time_ms(c, args.repeats) for c in calls] for _ in range(2)]
            best = [min(r[i] for r in runs) for i in range(len(calls))]
            (pts, sv, dp), (_, asv) = kgrad_block(S, d), kapply_block(S)
            W, gz, agz = -(-d // dp), -(-S // sv), -(-S // asv)
            row = {"S": S, "block": [pts, sv, dp], "windows": W, "grad_ms": best[0], "apply_ms": best[1], "runs_ms": runs,
                   "per_eval": (best[0] / (gz * W)) / (best[1] / agz), "over_W_applies": best[0] / (W * best[1])}
            if S == 1:
                row["pred_grad_ms"] = best[2]
            res["S"].append(row)
    _lib.kapply_fused_max(-1)
    dev.free_all()
    return res


def grad_paths_probe(n, d, dtype, args):
    rng = np.random.RandomState(0)
    X = rng.uniform(-10, 10, (n, d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(n)
    Xo = np.random.RandomState(2).uniform(-10, 10, (args.m, d))
    g = gp.GP(gp.GaussianKernel(1.0, 0.5 * np.sqrt(d)), X, y, s=1.0, dtype=dtype)
    res = {"n": n, "d": d, "dtype": dtype, "size": args.size, "features": args.features, "m": args.m}
    with Step("fit n = %d %s" % (n, dtype), args.step_timeout):
        res["log_lh"] = float(g.log_lh)
    with Step("value_and_grad against %d calls, n = %d d = %d %s" % (2 * d + 1, n, d, dtype), args.step_timeout):
        paths = g.sample_paths(args.size, seed=10, features=args.features)
        paths.value_and_grad(Xo)                                            # warm-up: code objects, scratch, the handle's buffers
        paths(Xo)
        step = 1e-5
        shifted = [Xo] + [Xo + sign * step * np.eye(d)[k] for k in range(d) for sign in (1.0, -1.0)]
        analytic, central = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            values, G = paths.value_and_grad(Xo)
            analytic.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            f = [paths(pts) for pts in shifted]
            central.append((time.perf_counter() - t0) * 1e3)
        num = np.stack([(f[1 + 2 * k] - f[2 + 2 * k]) / (2 * step) for k in range(d)], axis=2)
        res.update(value_and_grad_ms=min(analytic), central_ms=min(central), calls=2 * d + 1, ratio=min(central) / min(analytic),
                   runs_ms=[analytic, central], max_abs_grad=float(np.abs(G).max()), max_diff_to_central=float(np.abs(G - num).max()))
        paths.close()
    return res


def grad_main(args, Ss, shapes):
    res = {"device": _lib.device_info(0)["name"], "repeats": args.repeats, "mode": "grad",
           "clock": "primitive: HIP events on the null stream around `repeats` back-to-back calls after one warm-up, the kernels "
                    "alternating, the smaller of two such measurements; paths: the host clock, the best of three", "shapes": [], "paths": []}
    dev = Device()
    for dtype in args.dtypes.split(","):
        for n, d in shapes:
            res["shapes"].append(grad_shape_probe(dev, n, d, args.m, Ss, dtype, args))
    for dtype in args.dtypes.split(","):
        for n, d in shapes:
            res["paths"].append(grad_paths_probe(n, d, dtype, args))
    text = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    for sh in res["shapes"]:
        sys.stderr.write("n=%d d=%d m=%d %s\n   S   block     W    grad ms   apply ms  per eval  / W applies\n" % (sh["n"], sh["d"], sh["m"], sh["dtype"]))
        for r in sh["S"]:
            sys.stderr.write("%4d %9s %3d %10.3f %10.3f %9.2f %9.2f%s\n" % (r["S"], "x".join(str(v) for v in r["block"]), r["windows"], r["grad_ms"],
                             r["apply_ms"], r["per_eval"], r["over_W_applies"], "   pred_grad %.3f ms" % r["pred_grad_ms"] if "pred_grad_ms" in r else ""))
    for r in res["paths"]:
        sys.stderr.write("n=%d d=%d %s S=%d: value_and_grad %.2f ms, %d calls of paths(xo) %.2f ms, ratio %.1f\n"
                         % (r["n"], r["d"], r["dtype"], r["size"], r["value_and_grad_ms"], r["calls"], r["central_ms"], r["ratio"]))


def create_probe(n, d, args):
    rng = np.random.RandomState(0)
    X = rng.uniform(-10, 10, (n, d))
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(n)
    Xo = np.random.RandomState(2).uniform(-10, 10, (args.m, d))
    g = gp.GP(gp.GaussianKernel(1.0, 0.5 * np.sqrt(d)), X, y, s=1.0)
    res = {"n": n, "d": d, "dtype": "float64", "size": args.size, "features": args.features, "m": args.m}
    with Step("fit n = %d" % n, args.step_timeout):
        t0 = time.perf_counter()
        res["log_lh"] = float(g.log_lh)
        res["first_fit_s"] = time.perf_counter() - t0
    with Step("sample_paths(%d, features=%d)" % (args.size, args.features), args.step_timeout):
        g.sample_paths(2, seed=1, features=args.features).close()          # warm-up: code objects, scratch, block operators
        runs = []
        for rep in range(3):
            t0 = time.perf_counter()
            paths = g.sample_paths(args.size, seed=10 + rep, features=args.features)
            host_ms = (time.perf_counter() - t0) * 1e3
            runs.append(dict(paths.create_timing(), host_ms=host_ms))
            if rep < 2:
                paths.close()
        res["create_runs"] = runs
        res["create"] = min(runs, key=lambda r: r["total"])
    with Step("paths(xo) at m = %d" % args.m, args.step_timeout):
        paths(Xo)
        evals = []
        for _ in range(3):
            t0 = time.perf_counter()
            paths(Xo)
            evals.append((time.perf_counter() - t0) * 1e3)
        res["eval_host_ms"] = evals
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="apply", choices=["apply", "grad"])
    ap.add_argument("--shapes", default="65536x32,8192x3")
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--S", default=None, help="default: 1,4,8,16,32,64,128 (apply), 1,4,8,16,32,64 (grad)")
    ap.add_argument("--dtypes", default="float64,float32")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--create", default="", help="n x d of the creation measurement, e.g. 65536x32 (default: none)")
    ap.add_argument("--size", type=int, default=None, help="paths: default 64 (apply: --create), 8 (grad)")
    ap.add_argument("--features", type=int, default=1024)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    grad = args.mode == "grad"
    Ss = [int(v) for v in (args.S or ("1,4,8,16,32,64" if grad else "1,4,8,16,32,64,128")).split(",")]
    args.size = args.size if args.size is not None else (8 if grad else 64)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",") if s]
    if grad:
        return grad_main(args, Ss, shapes)
    res = {"device": _lib.device_info(0)["name"], "repeats": args.repeats,
           "clock": "HIP events on the null stream around `repeats` back-to-back calls after one warm-up; the routes alternate; "
                    "the smaller of two such measurements", "shapes": [], "fused_max": {}}
    dev = Device()
    for dtype in args.dtypes.split(","):
        for n, d in shapes:
            res["shapes"].append(shape_probe(dev, n, d, args.m, Ss, dtype, args))
        ok = [S for S in Ss if all(r["fused_ms"] <= r["gemm_ms"] for sh in res["shapes"] if sh["dtype"] == dtype
                                  for r in sh["S"] if r["S"] == S)]
        res["fused_max"][dtype] = max(ok) if ok else 0
    if args.create:
        n, d = (int(v) for v in args.create.split("x"))
        res["create"] = create_probe(n, d, args)
    text = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    for sh in res["shapes"]:
        sys.stderr.write("n=%d d=%d m=%d %s\n   S   fused ms    gemm ms\n" % (sh["n"], sh["d"], sh["m"], sh["dtype"]))
        for r in sh["S"]:
            sys.stderr.write("%4d %10.3f %10.3f\n" % (r["S"], r["fused_ms"], r["gemm_ms"]))
        sys.stderr.write("   S=1 fused %.3f ms, gpx_d_mean %.3f ms, ratio %.3f\n" % (sh["mean"]["fused_S1_ms"], sh["mean"]["mean_ms"], sh["mean"]["ratio"]))


if __name__ == "__main__":
    main()
