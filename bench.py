#!/usr/bin/env python3
"""bench.py -- GP fit + predict wall-clock on MI355X (BASELINE.json metric).

One "step" = one pass of the hot path over one synthetic data set, inputs
already resident in HBM:  kernel-matrix build (K + s^2 I, lower) -> Cholesky ->
forward/back solve (alpha) -> logdet + y^T alpha (log_lh) -> posterior mean at m
test points.  Workload at N=1: BASELINE config "N=65536, d=32 RBF fp64" (the
configuration the metric is quoted on; its 32 GiB matrix fits one 288 GB GPU).
With --gpus P > 1 the same problem (strong scaling) is factored over P ranks
with 1-D block-cyclic block columns and an RCCL broadcast of every factored
panel (gaussian_processes_amd/multi_gpu.py).

Prints ONE JSON line (rank 0) with the driver's contract (metric, value, unit,
higher_is_better, dtype, ms_per_step).  On one GPU a plain run does only that:
set-up, warm-up, the --steps timed steps (no per-launch events), the outputs
when --dump-outputs DIR is given, the line.  --full adds, on one GPU:
  roofline      -- the dominant kernel (fp64 MFMA gemm_nt: SYRK/GEMM updates of the
                   factorisation), achieved = sum of algorithmic flops of its
                   launches / sum of their HIP-event durations in the timed region
                   (the timed steps then carry the per-launch events; --no-prof drops them)
  check         -- K alpha = y on sampled rows of the timed result
  secondary     -- the other BASELINE configs, sizes and precisions, the gp.GP API path
                   (--no-secondary drops them)
  cpu_baseline  -- the oracle (CPU restatement of the reference's stage sequence)
                   timed on this host on a bounded sample and scaled stage by
                   stage (N^3 / N^2 / N) to the workload; N=1, rank 0 only
                   (--no-cpu-baseline drops it).

--dump-outputs DIR writes what the last timed step computed, as a caller of the
handle path receives it: DIR/log_lh.npy (float64, shape (1,)), DIR/alpha.npy
(K^-1 y, float64, shape (N,)) and DIR/mean.npy (posterior mean at the m test
points, in the run's dtype).  The inputs are seeded: the same arguments give the
same inputs in every run.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6     # 256 CU x 2.4 GHz x 128 flop/clk/CU
FP32_MFMA_PEAK_TFLOPS = 157.3


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--problem-n", dest="n", type=int, default=65536)
    ap.add_argument("--problem-d", dest="d", type=int, default=32)
    ap.add_argument("--problem-m", dest="m", type=int, default=1000)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--cpu-sample-n", type=int, default=32768)    # ONE sample at half the workload's N: ~80 s of host work and
                                                                  # ~30 GiB on the GPU box (round 6: the 12288 / 18432 samples of
                                                                  # round 5 extrapolated 2.1 - 2.5 x off -- the host BLAS is far from
                                                                  # its asymptotic rate there)
    ap.add_argument("--cpu-sample-n2", type=int, default=16384)   # a second, cheap sample (~12 s): two sizes fit the two-term model
                                                                  # t(N) = a N^3 + b N^2 of the O(N^3) stages (see cpu_baseline)
    ap.add_argument("--cpu-sample-n3", type=int, default=0)
    ap.add_argument("--cpu-budget-s", type=float, default=170.0,
                    help="host seconds the CPU samples may take together; a size predicted to overrun is skipped")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-prof", action="store_true", help="skip per-launch HIP-event profiling")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the side measurements (configs[1], [2], [4] and the gp.GP API path)")
    ap.add_argument("--launch-check", action="store_true",
                    help="rendezvous only (gloo, no GPU work): proves that `bench.py --gpus P` starts P ranks")
    ap.add_argument("--full", action="store_true",
                    help="one GPU: also the roofline (per-launch events in the timed steps), the residual check, the secondary "
                         "measurements and the CPU baseline; a plain run times the headline steps and nothing else")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's results (log_lh, alpha, mean) to DIR/<name>.npy (one GPU only)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and (args.gpus > 1 or os.environ.get("GPX_MG_REHEARSE") or os.environ.get("GPX_BENCH_FORCE_DIST")):
        ap.error("--dump-outputs is implemented for the single-GPU run only")
    return args


def synth(N, d, m, npdt):
    """SURVEY section 8(d) inputs (the oracle's synth_inputs, restated so that the timed
    path does not import the oracle)."""
    rng = np.random.RandomState(0)
    X = rng.uniform(-10, 10, (N, d))
    if d == 1:
        X = np.sort(X.ravel()).reshape(N, 1)
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.randn(N)
    Xo = np.random.RandomState(1).uniform(-10, 10, (m, d))
    return X.astype(npdt), y.astype(npdt), Xo.astype(npdt)


def sampled_row_residual(X, y, alpha, h, w, s, nrows=16):
    """max_i |K[r_i, :] alpha - y[r_i]| / max|y| on `nrows` sampled rows, K rebuilt here in float64
    numpy from the kernel's definition (gaussian_c.pyx:27-35, r^2 summed over the d inputs):
    a size-independent end-to-end check of build + factor + both solves on the timed workload."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    N = X.shape[0]
    rows = np.unique(np.concatenate([[0, 1, N // 2, N - 2, N - 1],
                                     np.random.RandomState(7).randint(0, N, max(0, nrows - 5))]))
    c1 = -0.5 / (w * w)
    c2 = 0.5 * np.sqrt(2.0 / np.pi) * h * h / w
    res = 0.0
    for r in rows:
        d2 = ((X - X[r]) ** 2).sum(1)
        e = c1 * d2
        k = np.where(e < -705.6238298100243, 0.0, c2 * np.exp(e))
        k[r] += s * s
        res = max(res, abs(float(k @ alpha) - float(y[r])))
    return res / max(1e-300, float(np.abs(y).max())), int(rows.size)


def _cpu_sample(orc, ns, d, m):
    """Oracle stage sequence at N = ns: seconds per stage (and the log_lh it produced)."""
    X, y, Xo = orc.synth_inputs(ns, d, m)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    o = orc.OracleGP("gaussian", (h, w), X, y, s)
    t = {}
    t0 = time.perf_counter(); o.Kxx; t["kmat"] = time.perf_counter() - t0
    t0 = time.perf_counter(); o.Lxx; t["potrf"] = time.perf_counter() - t0
    t0 = time.perf_counter(); o.inv_Kxx_y; t["solve"] = time.perf_counter() - t0
    t0 = time.perf_counter(); llh = o.log_lh; t["slogdet_lu"] = time.perf_counter() - t0
    t0 = time.perf_counter(); o.mean(Xo); t["mean"] = time.perf_counter() - t0
    return t, float(llh)


def _blas_info():
    """Which BLAS / LAPACK the reference's scipy / numpy calls run on here, and with how many threads."""
    info = []
    try:
        from threadpoolctl import threadpool_info
        for pool in threadpool_info():
            info.append({k: pool.get(k) for k in ("user_api", "internal_api", "version", "threading_layer", "architecture",
                                                  "num_threads")})
    except Exception:                  # noqa: BLE001 -- informational only
        pass
    return info


def cpu_baseline(N, d, m, sample_ns, budget_s=170.0):
    """Oracle stage sequence (the reference's own: C kernel loop, scipy cholesky / cho_solve, numpy slogdet LU, dot)
    on the host cores, on bounded samples (`sample_ns`, increasing), scaled stage by stage to N.

    ONE number: `value` scales the LARGEST sample with the stages' nominal exponents (N^2, N^3, N^2, N^3, N), i.e. it
    assumes the host keeps the per-stage rate it showed at that sample.  The rate is still rising there (64 BLAS
    threads are not saturated by a 24576^3 / 3 factorisation), so `value` is an upper estimate; `spread.low` is the
    same scaling with the exponents FITTED from the two largest samples (a lower estimate: it extrapolates the rise).
    Achieved GFLOP/s per O(N^3) stage and sample, and the BLAS build, are reported beside it."""
    from oracle import gp_oracle as orc
    blas = _blas_info()
    blas_threads = max([p.get("num_threads") or 1 for p in blas] or [os.cpu_count() or 1])
    ns_list = sorted(set(min(int(v), N) for v in sample_ns if v))
    _cpu_sample(orc, min(768, N), d, 8)                     # untimed: library loading / thread-pool start-up
    samples, llh = [], None
    skipped = []
    t_begin = time.perf_counter()
    for ns in ns_list:
        # a bounded sample (the contract: the default run finishes within a few minutes whatever the host): the next size is
        # predicted from the one before (measured on this pool's host: the N = 32768 sequence takes 3.6 x the N = 16384 one --
        # N^3 work at a rising BLAS rate; budgeted as (ratio of sizes)^3 / 2) and skipped when it would overrun
        if samples:
            n_prev, t_prev = samples[-1]
            predicted = sum(t_prev.values()) * (ns / float(n_prev)) ** 3 / 2.0
            if (time.perf_counter() - t_begin) + predicted > budget_s:
                skipped.append({"N": ns, "predicted_seconds": round(predicted, 1)})
                continue
        t, llh_s = _cpu_sample(orc, ns, d, m)
        if llh is None:
            llh = llh_s
        samples.append((ns, t))
    powers = {"kmat": 2.0, "potrf": 3.0, "solve": 2.0, "slogdet_lu": 3.0, "mean": 1.0}
    flops = {"potrf": lambda n: n ** 3 / 3.0, "slogdet_lu": lambda n: 2.0 * n ** 3 / 3.0}
    base_n, base_t = samples[-1]
    r = N / float(base_n)
    scaled = {k: base_t[k] * r ** powers[k] for k in powers}
    nominal = sum(scaled.values())
    # Round 6: the O(N^3) stages (LAPACK dpotrf, the LU of slogdet) are modelled as t(N) = a N^3 + b N^2 -- level-3 work
    # at the host's asymptotic rate plus the O(N^2) panel / synchronisation work that holds 64 threads back at small N
    # -- with a, b from the TWO largest in-run samples.  Scaling one sample by N^3 assumes the rate it ran at (389 GFLOP/s
    # at N = 32768 where the full-size run reached 587): 1.4 - 2.5 x too slow in rounds 5 - 6; the two-term fit from
    # N = 16384 / 32768 lands within a few per cent of the offline full-size measurement (extrapolated_over_measured).
    model = None
    if len(samples) >= 2:
        (n1, t1), (n2, t2) = samples[-2], samples[-1]
        model = {}
        for k in ("potrf", "slogdet_lu"):
            det = float(n1) ** 3 * float(n2) ** 2 - float(n2) ** 3 * float(n1) ** 2
            a3 = (t1[k] * float(n2) ** 2 - t2[k] * float(n1) ** 2) / det
            b2 = (float(n1) ** 3 * t2[k] - float(n2) ** 3 * t1[k]) / det
            if a3 > 0 and b2 >= 0:
                scaled[k] = a3 * float(N) ** 3 + b2 * float(N) ** 2
                model[k] = {"form": "a N^3 + b N^2", "a_N3": a3, "b_N2": b2,
                            "asymptotic_gflops": round((1.0 if k == "potrf" else 2.0) / 3.0 / a3 / 1e9, 1)}
            else:
                # the stage grew SLOWER than N^2 between the two samples (the host LU's thread scaling does that below
                # N ~ 32768): no two-term fit.  Bracket instead: rate held (N^3 from the largest sample) above, the
                # measured power law continued below; take the geometric mean and say so
                ex = max(1.0, min(3.0, float(np.log(max(t2[k], 1e-9) / max(t1[k], 1e-9)) / np.log(n2 / float(n1)))))
                hi_k, lo_k = t2[k] * r ** 3.0, t2[k] * r ** ex
                scaled[k] = float(np.sqrt(hi_k * lo_k))
                model[k] = {"form": "geometric mean of [power law N^%.2f continued, N^3 from the largest sample]" % ex,
                            "low": round(lo_k, 2), "high": round(hi_k, 2)}
    value = sum(scaled.values())
    fair = value - scaled["slogdet_lu"]
    fitted, low = None, None
    if len(samples) >= 2:
        (n1, t1), (n2, t2) = samples[-2], samples[-1]
        fitted = {k: float(np.log(max(t2[k], 1e-9) / max(t1[k], 1e-9)) / np.log(n2 / float(n1))) for k in ("potrf", "slogdet_lu", "kmat")}
        fp = dict(powers); fp.update({k: max(1.0, min(3.0, v)) for k, v in fitted.items()})
        low = sum(base_t[k] * r ** fp[k] for k in powers)
    cpu_model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    cpu_model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    out = {
        "value": round(value, 3), "unit": "s", "cores": int(blas_threads), "kind": "port",
        "spread": {"low": None if low is None else round(low, 3), "high": round(nominal, 3),
                   "meaning": "high = the largest sample scaled at nominal exponents (its rate held); low = exponents fitted from "
                              "the two largest samples (a power law: the rate keeps rising); value = the two-term model between them"},
        "two_term_model": model,
        "sample_budget_s": budget_s, "samples_skipped_over_budget": skipped,
        "os_cpu_count": os.cpu_count(), "cpu_model": cpu_model, "blas": blas,
        "sample_seconds": round(sum(sum(t.values()) for _, t in samples), 3),
        "fair_value": round(fair, 3),
        "log_lh_sample": llh,
        "samples": [{"N": ns, "seconds": {k: round(v, 3) for k, v in t.items()},
                     "gflops": {k: round(f(ns) / max(t[k], 1e-9) / 1e9, 1) for k, f in flops.items()}} for ns, t in samples],
    }
    if fitted is not None:
        out["fitted_exponents"] = {k: round(v, 3) for k, v in fitted.items()}
    # what stands between this host and running the workload itself: memory (K, L and the LU's copy as float64, plus
    # LAPACK work space: ~3.2 N^2 x 8 bytes) and time (the extrapolation itself) -- measured, not asserted
    need_gib = 3.2 * N * N * 8 / 2.0 ** 30
    try:
        host_gib = os.sysconf("SC_PHYS_PAGES") * os.sysconf("SC_PAGE_SIZE") / 2.0 ** 30
    except (ValueError, OSError, AttributeError):
        host_gib = None
    out["full_size_run"] = {"host_mem_gib": None if host_gib is None else round(host_gib, 1),
                            "needed_mem_gib": round(need_gib, 1), "estimated_seconds": round(value, 1),
                            "binding_limit": ("memory" if (host_gib is not None and host_gib < need_gib) else "time")}
    # `value` is what THIS run timed: the largest in-run sample scaled at nominal exponents (round 6: nothing in it depends
    # on a committed file).  Round 5 ran the workload itself ONCE at full size on a GPU box's host, off the timed bench
    # (tools/cpu_baseline_full.py -> profiles/r05_cpu_baseline_n65536.json): that measurement is carried beside it as
    # `value_measured_offline`, and `extrapolated_over_measured` says how far today's scaling is from it.
    out["extrapolated_value"] = out["value"]
    out["value_in_run"] = out["value"]
    out["value_is"] = ("timed in this run: the oracle stage sequence at N=%s, scaled to N=%d -- the O(N^3) stages by the two-term "
                       "model t = a N^3 + b N^2 fitted from the two samples, the others at their nominal exponents"
                       % (" and ".join(str(ns) for ns, _ in samples[-2:]), N)) if model else \
                      ("timed in this run: the N=%d sample of the oracle stage sequence scaled per stage at nominal exponents "
                       "to N=%d (an upper estimate while the host BLAS rate still rises with N)" % (base_n, N))
    try:
        mpath = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r05_cpu_baseline_n%d.json" % N)
        meas = json.load(open(mpath))
        if meas["N"] == N and meas["d"] == d and meas.get("reference_faithful_value_s"):
            same_cpu = meas["host"].get("cpu_model") == cpu_model and meas["host"].get("blas_threads") == blas_threads
            out["measured_full_size"] = {
                "file": "profiles/r05_cpu_baseline_n%d.json" % N, "seconds": meas["seconds"],
                "reference_faithful_s": meas["reference_faithful_value_s"], "fair_s": meas["fair_value_s"],
                "gflops": meas["gflops"], "host": {k: meas["host"].get(k) for k in ("cpu_model", "blas_threads", "mem_gib")},
                "same_cpu_model_and_threads_as_this_run": bool(same_cpu),
                "label": "measured offline on %s (%s BLAS threads), tools/cpu_baseline_full.py"
                         % (meas["host"].get("cpu_model"), meas["host"].get("blas_threads"))}
            out["extrapolated_over_measured"] = round(value / meas["reference_faithful_value_s"], 3)
            if same_cpu:
                out["value_measured_offline"] = round(meas["reference_faithful_value_s"], 3)
                out["fair_value_measured_offline"] = round(meas["fair_value_s"], 3)
    except (OSError, ValueError, KeyError):
        pass
    api = next((p for p in blas if p.get("user_api") == "blas"), {})
    out["sample"] = (
        "oracle stage sequence (C kernel loop 1 thread; scipy cholesky / cho_solve, numpy slogdet LU on %d threads of %s %s) at d=%d "
        "m=%d: %s; value = the samples scaled to N=%d (largest: N=%d; O(N^3) stages by t = a N^3 + b N^2 from two samples when there are two, else N^3) -- timed in this run (the full-size run "
        "needs ~%.0f GiB and ~%.0f s); potrf ran at %s GFLOP/s, the LU at %s; without the reference's redundant LU: %.1f s"
        % (blas_threads, api.get("internal_api", "BLAS"), api.get("version", "?"), d, m,
           "; ".join("N=%d: %s" % (ns, ", ".join("%s %.2fs" % kv for kv in t.items())) for ns, t in samples),
           N, base_n, need_gib, value,
           " / ".join("%.0f" % smp["gflops"]["potrf"] for smp in out["samples"]),
           " / ".join("%.0f" % smp["gflops"]["slogdet_lu"] for smp in out["samples"]), fair))
    if "measured_full_size" in out:
        mf = out["measured_full_size"]
        out["sample"] += (" | MEASURED at full size offline (%s): %.1f s reference-faithful, %.1f s without the LU (potrf %s GFLOP/s, LU %s)"
                          "; extrapolated / measured = %.2f"
                          % (mf["label"], mf["reference_faithful_s"], mf["fair_s"], mf["gflops"]["potrf"], mf["gflops"]["slogdet_lu"],
                             out["extrapolated_over_measured"]))
    return out


def _launch_once(nproc, extra_env):
    """Start `nproc` ranks of this script under torch.distributed.run (one per GPU, rendezvous on
    127.0.0.1); returns (the launcher's exit code, rank 0's JSON line or None)."""
    import socket
    import subprocess
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ)
    env.update(extra_env)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC only on this driver (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // nproc)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=None, text=True)
    line = None
    for out in proc.stdout:
        out = out.rstrip("\n")
        if out.startswith("{") and '"metric"' in out:
            line = out
        elif out:
            sys.stderr.write(out + "\n")                   # anything else a rank printed: keep stdout to one line
    rc = proc.wait()
    return rc, line


def self_launch(nproc):
    """`python bench.py --gpus P` from a plain shell: launch the ranks; when they end because a rank's watchdog fired
    (multi_gpu.Watchdog: communicator set-up or the first collective hung) start ONE more set of fresh child
    processes with the host-callback data plane (GPX_DIST_BACKEND=gloo: same C schedule, collectives staged through
    the host), so that the run still yields a labelled line.  This launcher process never touches the GPU; a process
    that did is never re-executed."""
    rc, line = _launch_once(nproc, {})
    if line is None and rc != 0 and os.environ.get("GPX_DIST_BACKEND", "nccl") != "gloo" and \
            not os.environ.get("GPX_BENCH_NO_RETRY"):
        sys.stderr.write("bench.py: the RCCL run ended with status %d and no result line; retrying ONCE in fresh "
                         "processes over the host-callback data plane\n" % rc)
        rc, line = _launch_once(nproc, {"GPX_DIST_BACKEND": "gloo"})
        if line is not None:
            try:
                obj = json.loads(line)
                obj["data_plane_fallback"] = ("first attempt over RCCL ended without a result (launcher status "
                                              "non-zero, see stderr); this line: host callbacks over gloo")
                line = json.dumps(obj)
            except ValueError:
                pass
    if line is not None:
        print(line)
        sys.stdout.flush()
    elif rc == 0:
        sys.stderr.write("bench.py: the ranks exited without printing a result line\n")
        rc = 1
    return rc


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus P`: become the launcher.  Nothing has touched the GPU yet
        # (no library loaded, no torch.cuda call), the ranks are CHILD processes, never an exec.
        raise SystemExit(self_launch(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    if args.launch_check:
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.tensor([float(rank + 1)], dtype=torch.float64)
        dist.all_reduce(t)
        dist.barrier()
        if rank == 0:
            print(json.dumps({"metric": "launch check (no GPU work)", "value": None, "n_gpus": world,
                              "launch_check": True, "rank_sum": float(t.item())}))
        dist.destroy_process_group()
        return
    from gaussian_processes_amd import _lib
    from gaussian_processes_amd.device import DeviceBuffer, Event, sync
    lib = _lib.load()
    if _lib.device_count() < 1:
        raise SystemExit("bench.py needs an MI355X: " + _lib.last_error())
    if os.environ.get("GPX_BENCH_SINGLE_DEVICE"):
        local_rank = 0
    _lib.check(lib.gpx_set_device(local_rank))

    N, d, m = args.n, args.d, args.m
    dtid = _lib.F64 if args.dtype == "f64" else _lib.F32
    npdt = np.float64 if args.dtype == "f64" else np.float32
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    params = np.array([h, w], dtype=np.float64)
    X, y, Xo = synth(N, d, m, npdt)

    if world == 1 and os.environ.get("GPX_MG_REHEARSE"):
        # GPX_MG_REHEARSE=rank,world: ONE process does that rank's share of a world-rank run of this workload on one GPU
        # (multi_gpu.rehearse_rank: its own panels, packs and updates through the product's C schedule; the panels it does
        # not own out of a resident single-GPU factor; every broadcast a delay that MODELS the transfer).  Not the headline
        # measurement: the line says "rehearsal" in `metric`.
        from gaussian_processes_amd import multi_gpu
        r_, w_ = (int(v) for v in os.environ["GPX_MG_REHEARSE"].split(","))
        nb_env = os.environ.get("GPX_POTRF_NB")
        out = multi_gpu.rehearse_rank(N, d, r_, w_, X.astype(np.float64), y.astype(np.float64), params, s, dtype_id=dtid,
                                      nb=int(nb_env) if nb_env else None,
                                      chunks=int(os.environ.get("GPX_MG_BCAST_CHUNKS", "4")),
                                      sag=1 if os.environ.get("GPX_MG_BCAST") == "sag" else 0, fits=max(2, args.steps),
                                      link_GBps=float(os.environ.get("GPX_MG_REHEARSE_GBPS", "100")))
        out.update({"metric": "REHEARSAL of one rank's share of a %d-GPU GP fit (measured compute, modelled transfer)" % w_,
                    "value": round(out["rank_step_s"], 4), "unit": "s", "n_gpus": 1, "higher_is_better": False})
        print(json.dumps(out))
        return
    if world > 1 or os.environ.get("GPX_BENCH_FORCE_DIST"):
        from gaussian_processes_amd import multi_gpu
        result = multi_gpu.bench_distributed(
            args, X, y, Xo, params, s, dtid,
            residual_check=lambda alpha: sampled_row_residual(X, y, alpha, h, w, s))
        if rank == 0:
            print(json.dumps(result))
        return

    # ---- single GPU: everything through the gpx_gp handle, inputs resident in HBM ----
    result = measure_single(args, lib, _lib, N, d, m, dtid, npdt, args.steps, args.warmup, local_rank,
                            prof_on=args.full and not args.no_prof, check=args.full, dump_dir=args.dump_outputs)
    if not args.full:
        print(json.dumps(result))
        return
    if not args.no_secondary and (N, d) != (8192, 8):
        result["secondary"] = secondary_measurements(args, lib, _lib, local_rank, result)
    if not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(N, d, m, (args.cpu_sample_n, args.cpu_sample_n2, args.cpu_sample_n3),
                                              budget_s=args.cpu_budget_s)
    print(json.dumps(result))


def secondary_measurements(args, lib, _lib, local_rank, headline):
    """The other BASELINE.json configs and the drop-in API path on the driver's clock, same process, after the timed
    headline region (a list; every entry names its config):
      configs[1]  N=8192  d=8  fp64, m=1024          handle path
      small_fits  N=2048 / 4096, d=8 fp64            handle path (the reference's own sizes are smaller still)
      configs[2]  N=32768 d=16 fp32, m=1024          handle path, with the fp32 trailing kernel's roofline fraction
      configs[4]  64 (and 8) restarts x N=8192 d=8   one lock-step gpx_gp_fit_batch call (mlii.BatchEvaluator)
      headline workload once more through gp.GP(...).log_lh / .mean(xo) -- the reference's own API"""
    out = []
    sec = measure_single(args, lib, _lib, 8192, 8, 1024, _lib.F64, np.float64, 10, 2, local_rank, prof_on=False)
    out.append({"name": "configs[1]", "config": sec["config"]["workload"], "value": sec["value"], "unit": "s",
                "stages_ms": sec["stages_ms"], "potrf_tflops": sec["potrf_tflops"],
                "potrf_frac_of_peak": sec["potrf_frac_of_peak"], "log_lh": sec["log_lh"], "check": sec["check"]})
    # the sizes the reference is used at are smaller still: the latency-bound end of the same path (fp64, d = 8, m = 1024)
    small = {"name": "small_fits", "unit": "s", "config": "handle path at N=2048 / 4096, d=8, fp64, m=1024 (chain-bound: one resident "
             "launch per 256-column panel)"}
    for n_small in (2048, 4096):
        sm = measure_single(args, lib, _lib, n_small, 8, 1024, _lib.F64, np.float64, 20, 3, local_rank, prof_on=False)
        small["n%d" % n_small] = {"value": sm["value"], "potrf_ms": sm["stages_ms"]["potrf"], "potrf_tflops": sm["potrf_tflops"],
                                  "log_lh": sm["log_lh"], "check": sm["check"]}
    small["value"] = small["n2048"]["value"]
    out.append(small)
    # (the per-launch HIP events behind `roofline` cost a few per cent at this size: the value is timed without them)
    sec = measure_single(args, lib, _lib, 32768, 16, 1024, _lib.F32, np.float32, 5, 2, local_rank, prof_on=False)
    prof = measure_single(args, lib, _lib, 32768, 16, 1024, _lib.F32, np.float32, 3, 1, local_rank, prof_on=True)
    out.append({"name": "configs[2]", "config": sec["config"]["workload"], "value": sec["value"], "unit": "s",
                "stages_ms": sec["stages_ms"], "potrf_tflops": sec["potrf_tflops"],
                "potrf_frac_of_peak": sec["potrf_frac_of_peak"], "roofline": prof["roofline"],
                "value_with_event_profiling": prof["value"], "log_lh": sec["log_lh"], "check": sec["check"]})
    out.append(measure_mlii(_lib))
    # ragged orders on the clock (round 6): N = 65000 (d = 32) next to the headline's 65536 and N = 8191 (d = 8) next to
    # configs[1]'s 8192 -- orders that are no multiple of any tile or panel width; potrf TF/s by N^3 / 3 and the time
    # per flop relative to the aligned neighbour
    rag = {"name": "ragged_sizes", "unit": "s",
           "config": "handle path, fp64: N=65000 d=32 m=1000 (beside N=65536) and N=8191 d=8 m=1024 (beside N=8192)"}
    aligned = {65000: (headline["stages_ms"]["potrf"], headline["config"]["N"]), 8191: (out[0]["stages_ms"]["potrf"], 8192)}
    for n_r, d_r, m_r, st_r, wu_r in ((8191, 8, 1024, 10, 2), (65000, 32, 1000, 2, 1)):    # (the small one first: not right behind the release of 35 GB)
        if n_r == 65000 and headline["config"]["N"] != 65536:
            continue
        r_ = measure_single(args, lib, _lib, n_r, d_r, m_r, _lib.F64, np.float64, st_r, wu_r, local_rank, prof_on=False)
        a_ms, a_n = aligned[n_r]
        per_flop = (r_["stages_ms"]["potrf"] / float(n_r) ** 3) / (a_ms / float(a_n) ** 3)
        rag["n%d" % n_r] = {"value": r_["value"], "potrf_ms": r_["stages_ms"]["potrf"], "potrf_tflops": r_["potrf_tflops"],
                            "potrf_frac_of_peak": r_["potrf_frac_of_peak"], "potrf_time_per_flop_over_aligned": round(per_flop, 4),
                            "log_lh": r_["log_lh"], "check": r_["check"]}
    rag["value"] = rag.get("n65000", rag["n8191"])["value"]
    out.append(rag)
    out.append(measure_periodic_build(lib, _lib))
    if headline["config"]["N"] >= 4096:
        out.append(measure_api(headline))
    return out


def measure_mlii(_lib, N=8192, d=8):
    """BASELINE configs[4]: 64 (lengthscale, variance, noise) restarts x N = 8192, one GP per GPU across 8 GPUs.  One GPU's
    share of that is 8 restarts; the whole table on one GPU is 64.  SURVEY 8(d) draws."""
    from gaussian_processes_amd import mlii
    X, y, _ = synth(N, d, 4, np.float64)
    rs = np.random.RandomState(2)
    w = rs.uniform(0.25, 2, 64) * np.sqrt(d)
    h = rs.uniform(0.5, 2, 64)
    sn = rs.uniform(0.5, 2, 64)
    thetas = np.column_stack([h, w, sn])
    res = {"name": "configs[4]", "config": "batched ML-II: restarts x N=%d d=%d fp64, lock-step gpx_gp_fit_batch" % (N, d),
           "unit": "s"}
    with mlii.BatchEvaluator(X, y) as ev:
        for rows in (64, 8):
            ev(thetas[:rows])                                      # warm: workspace allocation, first launches
            reps = 3 if rows == 64 else 10
            t0 = time.perf_counter()
            for _ in range(reps):
                llh = ev(thetas[:rows])
            sec = (time.perf_counter() - t0) / reps
            tfl = rows * (N ** 3 / 3.0) / sec / 1e12
            res["restarts_%d" % rows] = {"value": round(sec, 5), "ms_per_restart": round(sec / rows * 1e3, 3),
                                         "tflops_n3_over_3": round(tfl, 2), "frac_of_peak": round(tfl / FP64_MFMA_PEAK_TFLOPS, 4),
                                         "finite_rows": int(np.isfinite(llh).sum()),
                                         "minus_inf_rows_logdet_below_MIN": int(np.isneginf(llh).sum())}
        # value AND gradient of every restart (round 6: gpx_gp_fit_batch_grad -- the lock-step factorisation plus, per row,
        # K^-1 = L^-T L^-1 and the fused trace / quadratic-form pass: ~3 x the flops of the value alone)
        for rows in (64, 8):
            ev.value_and_grad(thetas[:rows])
            reps = 1 if rows == 64 else 3
            t0 = time.perf_counter()
            for _ in range(reps):
                llh, grad = ev.value_and_grad(thetas[:rows])
            sec = (time.perf_counter() - t0) / reps
            res["value_and_grad_%d" % rows] = {"value": round(sec, 5), "ms_per_restart": round(sec / rows * 1e3, 3),
                                                "tflops_n3": round(rows * float(N) ** 3 / sec / 1e12, 2),
                                                "finite_gradients": int(np.isfinite(grad).all(axis=1).sum())}
    # the ML-II driver on one GPU's share of config 5: L-BFGS-B from 8 of the SURVEY draws at once, all restarts in lock-step
    # (mlii.optimize: one gpx_gp_fit_batch_grad call per step for every restart still running), a few iterations
    t0 = time.perf_counter()
    opt = mlii.optimize(X, y, thetas[:8], maxiter=6)
    sec = time.perf_counter() - t0
    res["optimize_8"] = {"value": round(sec, 3), "maxiter": 6, "batched_calls": int(opt["batched_calls"]),
                         "function_evaluations": int(opt["nfev"].sum()),
                         "restarts_improved": int((opt["log_lh"] > opt["log_lh0"]).sum()),
                         "best_log_lh_start": float(np.max(opt["log_lh0"])), "best_log_lh_end": float(np.max(opt["log_lh"])),
                         "note": "unclamped log marginal likelihood (the reference's logdet < MIN clamp returns -inf at this n)"}
    res["value"] = res["restarts_64"]["value"]
    return res


def measure_periodic_build(lib, _lib, N=8192):
    """The periodic kernel-matrix build (gp/ext/periodic_c.pyx:18-30: one sin and one exp per entry, no clamp) at
    N = 8192, fp64: full square and lower tiles only, d = 1 (the reference's case) and d = 8; HIP events around 10
    launches each.  GB/s by SURVEY 8(d)'s accounting: N^2 * 8 bytes written per build (the lower-only build writes
    the tiles that touch the lower triangle and is still divided by N^2 * 8, as 8(d) says)."""
    from gaussian_processes_amd.device import DeviceBuffer, Event, sync
    res = {"name": "periodic_build", "unit": "ms",
           "config": "PeriodicKernel(1.1, 0.8, 2.3) K(x, x) + s^2 I at N=%d fp64 (gpx_d_kmat, kmat_kernel MODE periodic)" % N}
    prm = np.array([1.1, 0.8, 2.3])
    ld = N
    out = DeviceBuffer((N, ld), np.float64)
    for d in (1, 8):
        X, _, _ = synth(N, d, 4, np.float64)
        dX = DeviceBuffer.from_host(X)
        for tri_name, tri in (("full", _lib.FULL), ("lower", _lib.LOWER)):
            def build():
                _lib.check(lib.gpx_d_kmat(_lib.F64, _lib.KERNEL_PERIODIC, _lib.K, dX.ptr, N, dX.ptr, N, d, _lib.dptr(prm), 0.25,
                                          tri, out.ptr, ld, None))
            build(); sync()
            e0, e1 = Event(), Event()
            reps = 10
            e0.record()
            for _ in range(reps):
                build()
            e1.record(); e1.sync()
            ms = e0.elapsed_ms(e1) / reps
            res["d%d_%s" % (d, tri_name)] = {"ms": round(ms, 4), "GBps_N2T": round(N * N * 8 / (ms * 1e-3) / 1e9, 1)}
        dX.free()
    out.free()
    res["value"] = res["d1_lower"]["ms"]
    return res


def measure_api(headline):
    """The headline step through the drop-in class: gp.GP(GaussianKernel(h, w), x, y, s) -> set a parameter -> .log_lh,
    .mean(xo) with host arrays in and out (gp/gp.py:216-223, 337-367, 574-597), against the handle path above."""
    import gaussian_processes_amd as gp
    N, d, m = headline["config"]["N"], headline["config"]["d"], headline["config"]["m"]
    dtype = "float64" if headline["dtype"] == "f64" else "float32"
    X, y, Xo = synth(N, d, m, np.float64)
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    g = gp.GP(gp.GaussianKernel(h, w), X, y, s=s, dtype=dtype)
    float(g.log_lh); g.mean(Xo)                                   # warm (allocation, uploads)
    steps = 2
    t0 = time.perf_counter()
    for k in range(steps):
        g.set_param("h", h * (1.0 + (k + 1) * 1e-13))             # invalidates the memo: the next read refits
        llh = float(g.log_lh)
        mean = g.mean(Xo)
    sec = (time.perf_counter() - t0) / steps
    assert np.isfinite(llh) and np.isfinite(mean).all()
    return {"name": "api_path", "config": "headline workload through gp.GP(...).set_param / .log_lh / .mean(xo) (host arrays)",
            "value": round(sec, 4), "unit": "s", "steps": steps, "handle_path_value": headline["value"],
            "api_over_handle": round(sec / headline["value"], 4), "log_lh": llh}


def measure_single(args, lib, _lib, N, d, m, dtid, npdt, steps, warmup, local_rank, prof_on, check=True, dump_dir=None):
    from gaussian_processes_amd.device import DeviceBuffer, sync
    dtype_name = "f64" if dtid == _lib.F64 else "f32"
    h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
    params = np.array([h, w], dtype=np.float64)
    X, y, Xo = synth(N, d, m, npdt)
    dX, dy, dXo = DeviceBuffer.from_host(X), DeviceBuffer.from_host(y), DeviceBuffer.from_host(Xo)
    dmean = DeviceBuffer((m,), npdt)
    handle = ctypes.c_void_p()
    _lib.check(lib.gpx_gp_create(ctypes.byref(handle), dtid, _lib.KERNEL_GAUSSIAN, N, d))
    _lib.check(lib.gpx_gp_set_data_device(handle, dX.ptr, dy.ptr))
    A, lda, px, py, palpha, stream = (ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_void_p(),
                                      ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p())
    _lib.check(lib.gpx_gp_device_ptrs(handle, ctypes.byref(A), ctypes.byref(lda), ctypes.byref(px),
                                      ctypes.byref(py), ctypes.byref(palpha), ctypes.byref(stream)))

    def step():
        _lib.check(lib.gpx_gp_set_params(handle, _lib.dptr(params), float(s)))
        _lib.check(lib.gpx_gp_fit(handle, None))
        _lib.check(lib.gpx_d_mean(dtid, _lib.KERNEL_GAUSSIAN, dXo.ptr, m, px, N, d, _lib.dptr(params),
                                  palpha, dmean.ptr, stream))
        out = ctypes.c_double(0.0)
        _lib.check(lib.gpx_gp_log_lh(handle, ctypes.byref(out)))    # syncs the stream
        return out.value

    for _ in range(warmup):
        step()
    sync()
    if prof_on:
        _lib.check(lib.gpx_prof_enable(1))
    stage_ms = np.zeros(5)
    t0 = time.perf_counter()
    for _ in range(steps):
        llh = step()
        ms = (ctypes.c_float * 5)()
        _lib.check(lib.gpx_gp_last_timing(handle, ms))
        stage_ms += np.array(list(ms))
    sync()
    elapsed = time.perf_counter() - t0
    sec_per_step = elapsed / steps
    stage_ms /= steps

    prof = {}
    if prof_on:
        names = ["kmat", "gemm_trailing", "potrf_diag", "trsm_rows", "trsv", "mean", "reduce",
                 "gemm_panel_bn64", "gemm_generic", "gemm_panel_bn128", "gemm_trailing_bn64"]
        for cls, nm in enumerate(names):
            a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            _lib.check(lib.gpx_prof_read(cls, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
            prof[nm] = {"launches": a.value, "ms": b.value, "work": c.value}
        _lib.check(lib.gpx_prof_enable(0))

    mean_out = dmean.to_host()
    mean_host = mean_out.astype(np.float64)
    info = ctypes.c_int(0)
    _lib.check(lib.gpx_gp_info(handle, ctypes.byref(info)))
    assert info.value == 0 and np.isfinite(llh) and np.isfinite(mean_host).all()
    if check or dump_dir:
        alpha_host = np.empty(N, dtype=np.float64)
        _lib.check(lib.gpx_gp_get_alpha(handle, _lib.dptr(alpha_host)))
    check_out = None
    if check:
        # the timed result itself is checked: K alpha = y on sampled rows, outside the timed region
        residual, nres = sampled_row_residual(X, y, alpha_host, h, w, s)
        res_tol = 1e-9 if dtype_name == "f64" else 2e-3
        assert residual < res_tol, "sampled-row residual %.3e exceeds %.1e" % (residual, res_tol)
        check_out = {"sampled_rows": nres, "max_abs_residual_K_alpha_minus_y_over_max_y": residual,
                     "tolerance": res_tol}
    if dump_dir:
        # the last timed step's results as the handle path hands them to its caller
        os.makedirs(dump_dir, exist_ok=True)
        np.save(os.path.join(dump_dir, "log_lh.npy"), np.array([llh], dtype=np.float64))
        np.save(os.path.join(dump_dir, "alpha.npy"), alpha_host)
        np.save(os.path.join(dump_dir, "mean.npy"), mean_out)

    peak = FP64_MFMA_PEAK_TFLOPS if dtype_name == "f64" else FP32_MFMA_PEAK_TFLOPS
    roofline = None
    if prof.get("gemm_trailing", {}).get("ms", 0) > 0:
        g = prof["gemm_trailing"]
        achieved = g["work"] / (g["ms"] * 1e-3) / 1e12
        roofline = {"bound": "mfma",
                    "kernel": "gpx::gemm_nt_fast_kernel<%s, 128, 1, 0> (trailing SYRK updates of the factorisation)"
                              % ("double" if dtype_name == "f64" else "float"),
                    "achieved": round(achieved, 3), "peak": peak, "unit": "TFLOP/s",
                    "frac": round(achieved / peak, 4), "traffic": None,
                    "launches_per_step": g["launches"] / steps,
                    "avg_launch_ms": round(g["ms"] / g["launches"], 4),
                    "flops_per_step": g["work"] / steps}
        # the same fraction over ALL trailing-update launches of the factorisation -- the 128 x 128 class above plus the
        # short updates on 128 x 64 tiles (gemm_trailing_bn64) -- so that rounds which move launches between the two
        # classes stay comparable
        g64 = prof.get("gemm_trailing_bn64", {"launches": 0.0, "ms": 0.0, "work": 0.0})
        all_ms, all_work = g["ms"] + g64["ms"], g["work"] + g64["work"]
        roofline["all_trailing"] = {"achieved": round(all_work / (all_ms * 1e-3) / 1e12, 3),
                                    "frac": round(all_work / (all_ms * 1e-3) / 1e12 / peak, 4),
                                    "launches_per_step": (g["launches"] + g64["launches"]) / steps,
                                    "ms_per_step": round(all_ms / steps, 3), "flops_per_step": all_work / steps}
        # HBM-side bytes per launch of that kernel: PMC counters cannot be read from inside this process, so
        # the figure is the committed rocprofv3 --pmc measurement of THIS command and workload (two separate
        # passes, FETCH_SIZE with the gfx950 x2 correction + WRITE_SIZE; tools/profile_round.sh).  It is only
        # reported when it was taken with the GEMM source that is running now (sha256 of gpx_gemm.hip recorded
        # beside the counters) and the same number of launches per step; otherwise traffic is null and the stale
        # figure is labelled as such.
        if N == 65536 and d == 32 and dtype_name == "f64":
            try:
                import hashlib
                here = os.path.dirname(os.path.abspath(__file__))
                pmc_rel = next(rel for rel in (os.path.join("profiles", "r06_pmc", "traffic_n65536.json"),
                                               os.path.join("profiles", "r05_pmc", "traffic_n65536.json"),
                                               os.path.join("profiles", "r04_pmc", "traffic_n65536.json"),
                                               os.path.join("profiles", "r03_pmc", "traffic_n65536.json"),
                                               os.path.join("profiles", "r02_pmc", "traffic_n65536.json"))
                               if os.path.exists(os.path.join(here, rel)))
                with open(os.path.join(here, pmc_rel)) as f:
                    pmc = json.load(f)
                with open(os.path.join(here, "gaussian_processes_amd", "csrc", "gpx_gemm.hip"), "rb") as f:
                    sha = hashlib.sha256(f.read()).hexdigest()
                label = "bytes per launch (fetch corrected %.3e + write %.3e)" % (
                    pmc["fetch_bytes_per_launch_corrected"], pmc["write_bytes_per_launch"])
                same_schedule = abs(pmc.get("launches_per_step", 0) - roofline["launches_per_step"]) < 0.5
                if pmc.get("gemm_source_sha256") == sha and same_schedule:
                    roofline["traffic"] = round(pmc["traffic_bytes_per_launch"])
                    roofline["traffic_unit"] = label
                    roofline["traffic_over_algorithmic"] = round(pmc["traffic_over_algorithmic"], 2)
                else:
                    roofline["traffic_stale"] = {"value": round(pmc["traffic_bytes_per_launch"]), "unit": label,
                                                 "note": "measured with an earlier build (gpx_gemm.hip or the launch schedule changed)"}
                roofline["traffic_source"] = pmc_rel + " (rocprofv3 --pmc, offline)"
            except (OSError, KeyError, ValueError, StopIteration):
                pass
    potrf_tflops = (N ** 3 / 3.0) / (stage_ms[1] * 1e-3) / 1e12 if stage_ms[1] > 0 else None

    result = {
        "metric": "GP fit+predict wall-clock (kernel build + Cholesky + solve + log_lh + posterior mean)",
        "value": round(sec_per_step, 4), "unit": "s", "n_gpus": 1, "steps": steps,
        "warmup": warmup, "ms_per_step": round(sec_per_step * 1e3, 2),
        "higher_is_better": False, "scaling": "strong", "vs_baseline": None,
        "dtype": dtype_name, "data": "synthetic",
        "config": {"workload": "N=%d d=%d RBF(GaussianKernel) %s, m=%d test points, h=1 w=0.5*sqrt(d) s=1"
                               % (N, d, dtype_name, m),
                   "N": N, "d": d, "m": m, "parallelism": "1 GPU"},
        "stages_ms": {k: round(float(v), 3) for k, v in
                      zip(("kernel_build", "potrf", "solve", "logdet_dot", "fit_total"), stage_ms)},
        "potrf_tflops": round(potrf_tflops, 3) if potrf_tflops else None,
        "potrf_frac_of_peak": round(potrf_tflops / peak, 4) if potrf_tflops else None,
        "log_lh": llh,
        "check": check_out,
        "roofline": roofline,
        "kernels": {k: {"launches_per_step": v["launches"] / steps,
                        "ms_per_step": round(v["ms"] / steps, 3)} for k, v in prof.items()},
        "device": _lib.device_info(local_rank),
    }
    if prof.get("kmat", {}).get("ms", 0) > 0:
        result["kmat_write_GBps"] = round(prof["kmat"]["work"] / (prof["kmat"]["ms"] * 1e-3) / 1e9, 1)
    lib.gpx_gp_destroy(handle)
    for buf in (dX, dy, dXo, dmean):
        buf.free()
    return result


if __name__ == "__main__":
    main()
