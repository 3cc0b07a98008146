"""Test infrastructure for the distributed posterior covariance (gpx_mg_cov) and gp.DistributedGP: `world` ranks as
threads of one process on GPU 0 (the in-process collectives of _thread_world), a two-process gloo world, and the
conditioning-scaled tolerances of the golden GP records restated for the members DistributedGP offers."""
import os
import threading

import numpy as np

from _thread_world import ThreadCallbacks, _Shared
from oracle import gp_oracle as orc

C_COND = 16.0                      # the constant of tests/test_gpu_parity.py's golden-record bounds
_EPS = np.finfo(np.float64).eps


def run_ranks(world, body, timeout=120):
    """body(rank, callbacks) on `world` threads at once; returns the list of their results.  A rank that fails aborts the
    shared barrier (nobody waits for it for ever); the first real error is raised here."""
    shared = _Shared(world, timeout)
    out, errs = [None] * world, [None] * world

    def main(rank):
        try:
            out[rank] = body(rank, ThreadCallbacks(shared, rank))
        except BaseException as exc:         # noqa: BLE001
            errs[rank] = exc
            shared.barrier.abort()

    threads = [threading.Thread(target=main, args=(r,), name="gpx-cov-rank-%d" % r) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout + 60)
    alive = [t.name for t in threads if t.is_alive()]
    assert not alive, "ranks still running after the timeout: %s" % alive
    first = next((e for e in errs if e is not None and not isinstance(e, threading.BrokenBarrierError)), None) or \
        next((e for e in errs if e is not None), None)
    if first is not None:
        raise first
    return out


def ref_cov(kind, kparams, X, y, s, Xo):
    """The oracle's posterior covariance through a Cholesky solve (scipy cho_factor / cho_solve; the oracle's kernels)."""
    import scipy.linalg
    K = orc.kernel_matrix(kind, "K", X, X, kparams)
    K[np.diag_indices_from(K)] += s * s
    Kxox = orc.kernel_matrix(kind, "K", Xo, X, kparams)
    Kxoxo = orc.kernel_matrix(kind, "K", Xo, Xo, kparams)
    c = scipy.linalg.cho_factor(K, lower=True)
    alpha = scipy.linalg.cho_solve(c, y)
    return Kxoxo - Kxox @ scipy.linalg.cho_solve(c, Kxox.T), Kxox @ alpha, alpha


def check_record(g, rec):
    """log_lh, lh, inv_Kxx_y, mean and cov of `g` against a golden record, |got - ref| <= C_COND cond(Kxx) eps scale
    with the scales of tests/test_gpu_parity.py::_check_gp_record."""
    xo, y = rec["xo"], rec["y"]
    n = rec["x"].shape[0]
    Kinv, alpha, L = rec["inv_Kxx"], rec["inv_Kxx_y"], rec["Lxx"]
    tol = C_COND * float(np.linalg.cond(rec["Kxx"])) * _EPS
    amax, aabs = float(np.abs(alpha).max()), np.abs(alpha)

    def close(got, ref, scale, what):
        err = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))))
        bound = tol * max(float(scale), 1e-300)
        assert err <= bound, "%s: |got - ref| = %.3e exceeds C_COND cond eps scale = %.3e" % (what, err, bound)

    close(g.inv_Kxx_y, alpha, amax, "inv_Kxx_y")
    llh_scale = 0.5 * float(np.abs(y) @ aabs) + float(np.abs(np.log(np.diag(L))).sum()) + 0.5 * n * np.log(2 * np.pi)
    close(g.log_lh, rec["log_lh"], llh_scale, "log_lh")
    close(g.lh, rec["lh"], llh_scale * float(rec["lh"]), "lh")
    rs = float(np.abs(rec["Kxox"]).sum(1).max())
    close(g.mean(xo), rec["mean"], rs * amax, "mean")
    close(g.cov(xo), rec["cov"], np.abs(rec["Kxoxo"]).max() + rs * rs * np.abs(Kinv).max(), "cov")


def gloo_worker(rank, world, port, outdir):
    """One rank of a two-process gloo world: gp.DistributedGP(dist=...) with host-callback collectives, GPU 0."""
    import torch.distributed as dist
    import gaussian_processes_amd as gp
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        N, d, m = 1500, 3, 50
        X, y, Xo = orc.synth_inputs(N, d, m)
        h, w, s = 1.0, 0.5 * np.sqrt(d), 1.0
        g = gp.DistributedGP(gp.GaussianKernel(h, w), X, y, s=s, dist=dist, backend="callbacks", nb=256, device=0)
        res = {"log_lh": g.log_lh, "alpha": g.inv_Kxx_y, "mean": g.mean(Xo), "cov": g.cov(Xo),
               "world": g.native.world}
        g.params = np.array([1.3, 0.7 * np.sqrt(d), 0.8])          # a refit at new parameters
        res.update(log_lh2=g.log_lh, cov2=g.cov(Xo))
        g.close()
        np.savez(os.path.join(outdir, "rank%d.npz" % rank), **res)
    finally:
        dist.destroy_process_group()


def run_gloo_world(world, outdir):
    import socket
    import torch.multiprocessing as mp
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    mp.spawn(gloo_worker, args=(world, port, outdir), nprocs=world, join=True)
    return [np.load(os.path.join(outdir, "rank%d.npz" % r)) for r in range(world)]
