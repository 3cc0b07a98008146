"""bench.py's single-GPU line: a plain run times the headline and nothing else, --full adds the side figures,
--dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gp_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run_bench(*argv, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "GPX_MG_REHEARSE", "GPX_BENCH_FORCE_DIST"):
        env.pop(k, None)
    return subprocess.run([sys.executable, BENCH] + [str(a) for a in argv], env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=timeout)


def _one_line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_refuses_bad_arguments_before_any_work():
    r = _run_bench("--steps", "0")
    assert r.returncode == 2 and "--steps" in r.stderr and not r.stdout.strip()
    r = _run_bench("--gpus", "2", "--dump-outputs", "unused")
    assert r.returncode == 2 and "--dump-outputs" in r.stderr and not r.stdout.strip()


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_timed_step(tmp_path):
    N, d, m = 2048, 4, 64
    out_dir = tmp_path / "outputs"
    out = _one_line(_run_bench("--gpus", 1, "--problem-n", N, "--problem-d", d, "--problem-m", m, "--steps", 3, "--warmup", 1,
                               "--dump-outputs", out_dir))
    assert out["metric"].startswith("GP fit+predict wall-clock") and out["unit"] == "s" and out["dtype"] == "f64"
    assert out["higher_is_better"] is False and out["n_gpus"] == 1
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] >= 0
    # nothing but the headline: no per-launch events, no residual check, no side measurements
    assert out["roofline"] is None and out["kernels"] == {} and out["check"] is None
    assert "secondary" not in out and "cpu_baseline" not in out
    llh, alpha, mean = (np.load(str(out_dir / (nm + ".npy"))) for nm in ("log_lh", "alpha", "mean"))
    assert llh.dtype == np.float64 and llh.shape == (1,) and llh[0] == out["log_lh"]
    assert alpha.dtype == np.float64 and alpha.shape == (N,)
    assert mean.dtype == np.float64 and mean.shape == (m,)
    X, y, Xo = orc.synth_inputs(N, d, m)
    o = orc.OracleGP("gaussian", (1.0, 0.5 * np.sqrt(d)), X, y, 1.0)
    np.testing.assert_allclose(llh[0], o.log_lh, rtol=1e-10)
    np.testing.assert_allclose(alpha, o.inv_Kxx_y, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(mean, o.mean(Xo), rtol=1e-8, atol=1e-11)


@pytest.mark.gpu
def test_bench_full_run_keeps_the_check_and_the_per_launch_table():
    out = _one_line(_run_bench("--gpus", 1, "--problem-n", 8192, "--problem-d", 8, "--problem-m", 1024, "--steps", 2,
                               "--warmup", 1, "--full", "--no-secondary", "--no-cpu-baseline"))
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert out["check"]["sampled_rows"] == 16
    assert out["check"]["max_abs_residual_K_alpha_minus_y_over_max_y"] < out["check"]["tolerance"]
    assert out["kernels"]["kmat"]["launches_per_step"] >= 1
