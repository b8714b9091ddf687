"""bench.py's plain run: it times --steps updates and nothing else (the side measurements are behind --full), and
--dump-outputs writes what the last timed update computed, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("roofline", "roofline_env_step", "host", "host_enqueue_ms_per_update", "rollout_only", "env_only", "dense_form",
             "interior_policy", "shard_4096", "solow_4096", "trade16_gru_8192", "cpu_baseline", "strong_scaling", "comm")


def test_bench_offers_full_and_dump_outputs():
    p = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout


def test_bench_refuses_zero_steps():
    p = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--steps" in p.stderr and p.stdout.strip() == ""


def _plain_run(out_dir):
    env = dict(os.environ, GRL_BENCH_FORCE_DEVICE="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--envs", "256", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_bench_times_the_steps_and_dumps_the_last_update(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    j = _plain_run(a)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j
    assert j["steps"] == 3 and j["ms_per_step_spread"]["n"] == 3 and j["ms_per_step"] > 0
    assert j["value"] > 0 and j["dtype"] == "f32" and j["higher_is_better"] is True
    assert not [k for k in FULL_ONLY if k in j]
    names = sorted(f for f in os.listdir(a))
    assert {"params.npy", "update_stats.npy", "rollout_actions.npy", "rollout_values.npy", "rollout_rewards.npy", "rollout_y.npy",
            "rollout_adv.npy", "rollout_boot.npy", "swarm_x.npy", "swarm_xa.npy"} <= set(names)
    assert sum(os.path.getsize(a / f) for f in names) <= 64 * 10 ** 6
    first = {f[:-len(".npy")]: np.load(a / f) for f in names}
    assert all(v.dtype in (np.float32, np.float64) for v in first.values())
    assert first["params"].shape == (2210213,) and np.isfinite(first["params"]).all()
    assert first["rollout_actions"].shape == (20, 2560, 2) and first["swarm_x"].shape == (256, 80, 2)
    st = first["update_stats"]
    assert st.shape == (4,) and np.isfinite(st).all() and st[3] > 0
    # the same arguments, the same inputs: a second run computes the same update
    _plain_run(b)
    assert sorted(os.listdir(b)) == names
    for k, v in first.items():
        np.testing.assert_allclose(np.load(b / (k + ".npy")), v, rtol=1e-5, atol=1e-6, err_msg=k)
