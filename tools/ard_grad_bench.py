"""tools/ard_grad_bench.py [N d reps] -- gpx_gp_dloglh_dtheta of the Gaussian ARD family beside the isotropic Gaussian
family on the same data in the same run (diagnostic).  Per family: the median host time of the call on a
fitted handle (the call synchronises), alternating the two families, and the gradient's reduction kernel alone
(gpx_prof_*, class GPX_PROF_REDUCE, in a pass of its own)."""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_processes_amd as gp
from gaussian_processes_amd import _lib

N, d, reps = (int(v) for v in (sys.argv[1:4] + ["8192", "32", "9"][len(sys.argv) - 1:]))
dtype = sys.argv[4] if len(sys.argv) > 4 else "float64"
rng = np.random.RandomState(0)
X = rng.uniform(-1, 1, (N, d))
y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(N)
w = rng.uniform(0.3, 3.0, d)
lib = _lib.load()
fam = {"gaussian_ard": gp.GP(gp.GaussianARDKernel(1.3, w), X, y, s=0.7, dtype=dtype),
       "gaussian": gp.GP(gp.GaussianKernel(1.3, float(np.exp(np.log(w).mean()))), X, y, s=0.7, dtype=dtype)}
handles, outs = {}, {}
for name, g in fam.items():
    handles[name] = g._fit_pd().handle
    outs[name] = np.empty(len(g.params))


def call(name):
    t0 = time.perf_counter()
    _lib.check(lib.gpx_gp_dloglh_dtheta(handles[name], _lib.dptr(outs[name])))
    return (time.perf_counter() - t0) * 1e3


for _ in range(2):                                           # warm-up: code objects, the workspaces, the block operators
    for name in fam:
        call(name)
times = {name: [] for name in fam}
for _ in range(reps):
    for name in fam:
        times[name].append(call(name))
res = {"N": N, "d": d, "dtype": dtype, "reps": reps, "device": _lib.device_info(0)["name"]}
for name in fam:
    t = np.array(times[name])
    res[name] = {"call_ms_median": float(np.median(t)), "call_ms_min": float(t.min()), "call_ms_max": float(t.max())}
    _lib.check(lib.gpx_prof_enable(1))
    call(name)
    launches, ms, work = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    _lib.check(lib.gpx_prof_read(6, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(work)))      # GPX_PROF_REDUCE
    _lib.check(lib.gpx_prof_enable(0))
    res[name]["reduce_kernel_ms"] = ms.value / max(launches.value, 1.0)
    res[name]["reduce_launches"] = launches.value
res["ratio_call"] = res["gaussian_ard"]["call_ms_median"] / res["gaussian"]["call_ms_median"]
print(json.dumps(res))
