"""bench.py end to end on a reduced config-M shape: the driver's JSON contract (one line, the keys
the round-end bench reads, roofline + RMSE window objects with --full; the lean line and the dumped
outputs without).  Runs in a child process like the driver."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    cmd = [sys.executable, os.path.join(REPO, "bench.py")] + list(args)
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("config", ["M", "mesh"])
def test_bench_line_contract(gpu_ready, config):
    out = run_bench("--full", "--config", config, "--steps", "1", "--warmup", "0", "--res", "64", "--spp", "16",
                    "--no-cpu-baseline", "--rmse-lanes", "4096")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in out, k
    assert out["value"] > 0 and out["scaling"] == "strong" and out["n_gpus"] == 1
    assert out["roofline"]["achieved"] > 0 and 0 < out["roofline"]["frac"] < 1
    assert out["rmse_vs_oracle"]["rmse"] < 1e-4
    assert out["config"]["workload"].startswith(config + ":")


def test_plain_bench_line_and_dumped_outputs(gpu_ready, amvpt_mod, tmp_path):
    """Without --full: the headline keys only (no instrumented frame, oracle or CPU baseline), --steps timed
    steps, and --dump-outputs writes the RGBW ImageBlock of the last timed step -- the frame amvpt.render
    gives for the same scene, up to the film's float-atomic summation order (relative 1e-5 of the film scale,
    as test_gpu_multi.py)."""
    defines = dict(res=64, spp=16, gx=4, gy=2, reuse=8, adaptive=0)
    out = run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump"),
                    *[a for k, v in defines.items() if k != "adaptive" for a in ("--" + k, str(v))])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in out, k
    for k in ("roofline", "cpu_baseline", "rmse_vs_oracle", "counters"):
        assert k not in out, k
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    lanes = out["config"]["samples_per_gpu_per_step"]
    assert abs(out["value"] - lanes / out["ms_per_step"] / 1e3) <= 2e-3 * out["value"]
    assert os.listdir(tmp_path / "dump") == ["film.npy"]
    film = np.load(tmp_path / "dump" / "film.npy")
    assert film.dtype == np.float32 and film.shape == (2 * 64, 4 * 64, 4)
    s = amvpt_mod.load_file(os.path.join(REPO, "scenes", "cbox_grid.xml"), **defines)
    ref = amvpt_mod.render(s, raw=True)
    assert np.abs(film - ref).max() <= 1e-5 * np.abs(ref).max()
