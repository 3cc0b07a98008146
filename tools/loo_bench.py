"""tools/loo_bench.py -- time diag(K^-1) by the leave-one-out sweep against the explicit inverse.

    python tools/loo_bench.py --route loo [--n 8192] [--d 32] [--chunk-rows 0]      # gpx_gp_inv_diag
    python tools/loo_bench.py --route inv [--n 8192] [--d 32]                       # np.diag(g.inv_Kxx)

One route per process, fp64, one JSON object on stdout.  A warm-up call, a refit (the handle drops its diagonal with the
factor), then ONE timed call between two HIP events on the handle's own stream: the time covers the device work and the
download the route ends in, not numpy's work on the result.  `peak_bytes` is the largest drop of free HBM below its level
before the timed call, polled from a second host thread every few milliseconds while the call runs.
"""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["loo", "inv"], required=True)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--chunk-rows", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=300, help="seconds; the process exits with status 124 beyond it")
    args = ap.parse_args()
    dog = threading.Timer(args.timeout, lambda: os._exit(124))
    dog.daemon = True
    dog.start()

    lib = _lib.load()
    n, d = args.n, args.d
    X, y, _ = orc.synth_inputs(n, d, 1)
    g = gp.GP(gp.GaussianKernel(1.0, 0.5 * np.sqrt(d)), X, y, s=1.0)
    out = np.empty(n) if args.route == "loo" else np.empty((n, n))

    def call(handle):
        if args.route == "loo":
            _lib.check(lib.gpx_gp_inv_diag(handle, args.chunk_rows, _lib.dptr(out)))
        else:
            _lib.check(lib.gpx_gp_get_inv_Kxx(handle, _lib.dptr(out), n))

    call(g._fit_pd().handle)                             # warm-up
    g.s = 2.0
    g.log_lh
    g.s = 1.0
    handle = g._fit_pd().handle                          # a new factor: nothing of the warm-up is kept
    fit_ms = g.fit_timing()["total"]
    stream = ctypes.c_void_p()
    _lib.check(lib.gpx_gp_device_ptrs(handle, None, None, None, None, None, ctypes.byref(stream)))
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        _lib.check(lib.gpx_event_create(ctypes.byref(e)))
    free0, low, stop = _lib.mem_free(), [None], threading.Event()

    def poll():
        low[0] = _lib.mem_free()
        while not stop.is_set():
            low[0] = min(low[0], _lib.mem_free())
            time.sleep(0.003)

    t = threading.Thread(target=poll)
    t.start()
    _lib.route_reset()
    _lib.check(lib.gpx_event_record(ev[0], stream))
    call(handle)
    _lib.check(lib.gpx_event_record(ev[1], stream))
    _lib.check(lib.gpx_event_sync(ev[1]))
    stop.set()
    t.join()
    ms = ctypes.c_float(0)
    _lib.check(lib.gpx_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
    kii = out if args.route == "loo" else np.diag(out)
    print(json.dumps({"route": args.route, "n": n, "d": d, "dtype": "float64", "ms": round(ms.value, 3),
                      "fit_ms": round(float(fit_ms), 3), "chunks": _lib.route_count(_lib.ROUTE_LOO_CHUNK),
                      "trsm_ops": _lib.route_count(_lib.ROUTE_TRSM_OPS), "peak_bytes": int(free0 - low[0]),
                      "free_before": int(free0), "kii_sum": float(np.sum(kii)), "kii_min": float(np.min(kii)),
                      "device": _lib.device_info(0)["name"]}))
    for e in ev:
        lib.gpx_event_destroy(e)


if __name__ == "__main__":
    main()
