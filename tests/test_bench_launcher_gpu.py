"""`python bench.py --gpus N` must launch its own ranks.  The N > 1 form needs N GPUs; the same launcher
path (bench.py -> torch.distributed.run -> one rank per GPU -> RCCL process group -> evaluate_sharded -> one JSON line from
rank 0) is exercised here with a world of ONE rank on the dp64 workload of the tiny configuration."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_self_launch_world1_dp64_tiny(hip_lib, cuda):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--spawn", "--workload", "dp64", "--model", "tiny",
           "--dp-images", "16", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-roofline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["scaling"] == "strong" and d["value"] > 0
    assert d["config"]["workload"].startswith("dp64") and d["config"]["images_per_step"] == 16


@pytest.mark.gpu
def test_bench_plain_run_b1_tiny_dumps_outputs(hip_lib, cuda, tmp_path):
    """A plain run times exactly --steps steps, leaves every --full leg out, and --dump-outputs writes the last step's result."""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--model", "tiny", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "images/s"
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]  # one image per step at N = 1
    for k in ("cpu_baseline", "roofline", "variant_fp8", "dp64_one_gpu", "free_running", "parity_vs_oracle_full_depth"):
        assert d[k] is None, k
    c, m = np.load(tmp_path / "pred_contact_3d.npy"), np.load(tmp_path / "pred_masks.npy")
    assert c.dtype == np.float32 and c.shape == (1, 6890) and np.isfinite(c).all() and ((c >= 0) & (c <= 1)).all()
    assert m.dtype == np.float32 and m.ndim == 3 and m.shape[0] == 4 and np.isfinite(m).all()
    assert np.load(tmp_path / "output_ids.npy").dtype == np.float64
