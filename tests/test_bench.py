"""bench.py's plain run (the headline only, exactly --steps timed steps), its --dump-outputs files, and --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

FULL_ONLY = ("median_run_kernel_ms", "whole_episode", "roofline", "policy_in_loop", "scaling_in_n", "many_steps_per_call",
             "async_groups", "cpu_baseline", "restarts_out_of_lockstep")


def run_bench(*args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:]
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])


def test_dump_outputs_samples_envs_beyond_the_budget(tmp_path):
    rs = np.random.RandomState(1)
    arrays = {"obs": rs.rand(1000, 30).astype(np.float32), "reward": rs.rand(1000).astype(np.float32),
              "done": (rs.rand(1000) < 0.1).astype(np.float32)}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    for name, a in arrays.items():
        assert np.array_equal(np.load(str(tmp_path / "all" / (name + ".npy"))), a)
    assert not (tmp_path / "all" / "env_index.npy").exists()

    budget = 64 * 1024
    for rank in (0, 1):
        bench.dump_outputs(str(tmp_path / "part"), arrays, rank=rank, world=2, budget=budget)
    files = sorted(os.listdir(str(tmp_path / "part")))
    assert files == sorted("%s_rank%d.npy" % (n, r) for n in ("obs", "reward", "done", "env_index") for r in (0, 1))
    assert sum(os.path.getsize(str(tmp_path / "part" / f)) for f in files) <= budget
    idx = np.load(str(tmp_path / "part" / "env_index_rank0.npy"))
    assert idx.dtype == np.float64 and len(idx) > 100 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(str(tmp_path / "part" / "env_index_rank1.npy")))   # the sample is fixed
    for name, a in arrays.items():
        assert np.array_equal(np.load(str(tmp_path / "part" / (name + "_rank0.npy"))), a[idx.astype(np.int64)])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_same_outputs_twice(tmp_path):
    args = ["--gpus", "1", "--envs", "8192", "--steps", "30", "--warmup", "5"]
    lines = [run_bench(*(args + ["--dump-outputs", str(tmp_path / d)])) for d in ("a", "b")]
    for out in lines:
        assert out["steps"] == out["timed_steps"] == 30 and out["warmup"] == 5
        assert out["repeats"] == 1 and out["runs_ms_per_step"] == [out["ms_per_step"]]
        assert out["value"] == pytest.approx(8192 / (out["ms_per_step"] * 1e-3), rel=1e-9)
        assert out["window"]["first_step_of_episode"] == 5
        assert out["unit"] == "env steps/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
        assert not [k for k in FULL_ONLY if k in out]
    shapes = {"obs": (8192, 30), "reward": (8192,), "done": (8192,)}
    for name, shape in shapes.items():
        a, b = (np.load(str(tmp_path / d / (name + ".npy"))) for d in ("a", "b"))
        assert a.dtype == np.float32 and a.shape == shape and np.all(np.isfinite(a))
        assert np.array_equal(a, b), name
    assert sorted(os.listdir(str(tmp_path / "a"))) == sorted(n + ".npy" for n in shapes)
    assert np.any(np.load(str(tmp_path / "a" / "obs.npy")) != 0)


@pytest.mark.gpu
def test_full_run_keeps_the_supplementary_figures():
    out = run_bench("--gpus", "1", "--envs", "8192", "--steps", "30", "--warmup", "5", "--full", "--no-cpu-baseline", "--no-pmc",
                    "--no-policy")
    assert out["timed_steps"] == 30 and out["repeats"] == 3 and len(out["runs_ms_per_step"]) == 3
    assert out["whole_episode"]["episodes"] == 3 and out["whole_episode"]["value"] > 0
    assert out["roofline"]["kernel"].startswith("send_kernel") and out["roofline"]["kernel_ms"] > 0
    assert out["median_run_kernel_ms"]["steps_with_events"] > 0
    assert out["cpu_baseline"] is None and out["config"]["packets_per_env_step"] > 0
