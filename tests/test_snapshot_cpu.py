"""Snapshot and restore, what can be checked without a GPU: the Python-side snapshot object survives a file, and the three entry
points refuse a NULL handle."""
import io

import torch

import pcc_rl_amd
from pcc_rl_amd import native


def test_env_snapshot_round_trips_through_torch_save():
    data = torch.arange(4096, dtype=torch.int64).to(torch.uint8)
    config = {"n_envs": 777, "n_senders": 1, "history_len": 10, "features": ["sent latency inflation", "latency ratio", "send ratio"],
              "seed": 5, "env_gid_base": 0, "ring_capacity": 32768, "ring_pools": [2, 8, 32], "max_steps": 30, "delta_scale": 0.025,
              "use_cwnd": False, "latency_noise": None, "loss_trace": False, "link_params": False}
    snap = pcc_rl_amd.EnvSnapshot(data, 12, True, config)
    f = io.BytesIO()
    torch.save({"env": snap, "iters_done": 3}, f)
    f.seek(0)
    back = torch.load(f)
    assert back["iters_done"] == 3
    got = back["env"]
    assert isinstance(got, pcc_rl_amd.EnvSnapshot)
    assert got.data.dtype == torch.uint8 and torch.equal(got.data, data)
    assert (got.t, got.was_reset, got.config) == (12, True, config)
    moved = got.to("cpu")
    assert torch.equal(moved.data, data) and moved.config == config and moved.nbytes == 4096
    groups = pcc_rl_amd.GroupedEnvSnapshot([snap, snap]).to("cpu")
    assert len(groups.groups) == 2 and groups.groups[1].t == 12
    # SimulatedNetworkEnv's own state is a field: to() and a file carry it
    adapter = {"hist": [[0.0, 1.0, 1.0]] * 10, "steps_taken": 4, "reward_sum": 1.5, "reward_ewma": 0.0, "episodes_run": 0, "run_dur": 0.25,
               "events": [{"Name": "Step", "Time": 1, "Reward": 0.5}]}
    with_state = pcc_rl_amd.EnvSnapshot(data, 4, True, config, adapter)
    assert with_state.to("cpu").adapter == adapter and snap.to("cpu").adapter is None
    f = io.BytesIO()
    torch.save(with_state, f)
    f.seek(0)
    assert torch.load(f).adapter == adapter


def test_header_is_read_only_from_a_known_format():
    import numpy as np
    import pytest
    head = np.zeros(472, dtype=np.uint8)
    head[:8] = np.frombuffer(b"PCCSNAP1", dtype=np.uint8)
    head[8:16] = np.array([1, 472], dtype=np.uint32).view(np.uint8)
    head[472 - 24:472 - 8] = np.array([77, 4096], dtype=np.uint64).view(np.uint8)
    data = torch.zeros(4096, dtype=torch.uint8)
    data[:472] = torch.from_numpy(head)
    snap = pcc_rl_amd.EnvSnapshot(data, 0, True, {})
    assert snap.header() == {"ring_records": 77, "total_bytes": 4096, "truncated": False, "header_bytes": 472}
    for at, value in ((0, ord("Q")), (8, 2)):   # another magic, another version
        bad = data.clone()
        bad[at] = value
        with pytest.raises(ValueError):
            pcc_rl_amd.EnvSnapshot(bad, 0, True, {}).header()


def test_entry_points_refuse_a_null_handle():
    L = native.lib()
    assert L.pcc_snapshot_bytes(None, None) == -1 and b"NULL" in L.pcc_last_error()
    assert L.pcc_snapshot(None, None, 0, None) == -1 and b"NULL" in L.pcc_last_error()
    assert L.pcc_restore(None, None, 0, None) == -1 and b"NULL" in L.pcc_last_error()
