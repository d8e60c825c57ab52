"""The episode ledger, the part that needs no GPU (include/pcc_policy.h: pcc_episode_update_pop and its stand-alone form; DESIGN.md
section 21): the numpy restatement of the contract (tests/models/episode_ledger_model.py) against a plain Python loop that lists
every episode, the three symbols, every refusal of the host side, the compiler's resource report of the two kernels, and what
the Python layer refuses or leaves as it was."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import episode_ledger_model as model  # noqa: E402

from pcc_rl_amd import native  # noqa: E402
from pcc_rl_amd.episodes import EpisodeLedger, column_index, summarise  # noqa: E402
from pcc_rl_amd.native import lib  # noqa: E402
from pcc_rl_amd.ppo import PPO, PopulationPPO  # noqa: E402

EP_SYMBOLS = {"pcc_episode_scratch_doubles": 3, "pcc_episode_update_pop": 16, "pcc_episode_update": 15}


def random_rows(rng, T, N, p, scale=(1.0, 1e3, 1e-3)):
    reward = (3.0 * rng.standard_normal((T, N))).astype(np.float32)
    done = (rng.random((T, N)) < p).astype(np.uint8)
    steps = rng.standard_normal((T, N, model.STEP_COLS)) * np.resize(np.array(scale), model.STEP_COLS)
    return reward, done, steps


# ------------------------------------------------------------------------------------------ the contract, restated in numpy
@pytest.mark.parametrize("p", [0.0, 0.05, 0.5, 1.0])
def test_the_restatement_lists_the_episodes_of_a_plain_loop(p):
    rng = np.random.default_rng(int(p * 100) + 1)
    T, N, K, cols = 23, 12, 3, [6, 0, 17]
    reward, done, steps = random_rows(rng, T, N, p)
    led = model.Ledger(N, K, cols)
    new = led.update(reward, done, steps)
    want, left, left_len = model.plain_loop(reward, done, steps, cols)
    got = sorted((i, n, tuple(v)) for m in range(K) for (i, n, v) in new[m])
    assert got == sorted((i, n, tuple(v)) for (i, t, n, v) in want)
    assert all(i // (N // K) == m for m in range(K) for (i, n, v) in new[m])
    assert np.array_equal(led.carry, left) and np.array_equal(led.carry_len, left_len)
    for i in range(N):   # last: the env's latest episode of the loop's list
        mine = [e for e in want if e[0] == i]
        if mine:
            assert led.last[i].tolist() == mine[-1][3] and led.last_len[i] == mine[-1][2]
        else:
            assert not led.last[i].any() and led.last_len[i] == 0
    for m in range(K):
        mine = [e for e in want if e[0] // (N // K) == m]
        row = led.totals[m]
        if not mine:
            assert not row.any()
            continue
        assert row[0] == len(mine) and row[1] == sum(e[2] for e in mine)
        for c in range(led.C):
            v = [e[3][c] for e in mine]
            assert row[2 + 4 * c] == math.fsum(v) and row[3 + 4 * c] == math.fsum(a * a for a in v)
            assert row[4 + 4 * c] == min(v) and row[5 + 4 * c] == max(v)
    assert int(led.totals[:, 0].sum()) == int(done.sum())
    assert int(led.totals[:, 1].sum()) + int(led.carry_len.sum()) == T * N     # every step is in an episode or in a carry


def test_the_restatement_splits_and_carries():
    """Two calls over a split of the rows leave the bits of one call; the carry of the first is where the second goes on."""
    rng = np.random.default_rng(7)
    T, N, cols = 17, 10, [6]
    reward, done, steps = random_rows(rng, T, N, 0.2)
    one = model.Ledger(N, 2, cols)
    one.update(reward, done, steps)
    for T1 in (1, 8, 16):
        two = model.Ledger(N, 2, cols)
        two.update(reward[:T1], done[:T1], steps[:T1])
        mid, mid_len = two.carry.copy(), two.carry_len.copy()
        two.update(reward[T1:], done[T1:], steps[T1:])
        for name in ("carry", "carry_len", "last", "last_len"):
            assert np.array_equal(getattr(one, name), getattr(two, name)), (T1, name)
        assert np.array_equal(one.totals[:, :2], two.totals[:, :2])
        assert np.array_equal(one.totals[:, 4::4], two.totals[:, 4::4]) and np.array_equal(one.totals[:, 5::4], two.totals[:, 5::4])
        want, left, left_len = model.plain_loop(reward[T1:], done[T1:], steps[T1:], cols, mid, mid_len)
        assert np.array_equal(two.carry, left) and np.array_equal(two.carry_len, left_len)


def test_the_restatement_keeps_a_row_without_episodes_and_the_padding():
    led = model.Ledger(4, 2, [], totals_stride=9)
    led.totals[:] = 5.0
    reward = np.ones((3, 4), dtype=np.float32)
    done = np.zeros((3, 4), dtype=np.uint8)
    done[2, 0] = 1
    led.update(reward, done)
    assert led.totals[1].tolist() == [5.0] * 9                       # no finished episode: untouched
    assert led.totals[0].tolist() == [6.0, 8.0, 8.0, 14.0, 3.0, 5.0, 5.0, 5.0, 5.0]   # merged into the row; the padding stays
    b_sum, b_sq = model.sum_bounds(led.episodes[0], 1, prior=[5.0] * 6)
    assert b_sum == [2 * 2.0 ** -52 * 8.0] and b_sq == [2 * 2.0 ** -52 * 14.0]


def test_summary_of_totals_rows():
    s = summarise([[2.0, 30.0, 10.0, 58.0, 3.0, 7.0], [0.0] * 6], ["reward_f32"])
    assert s["episodes"] == [2, 0] and s["mean_length"][0] == 15.0 and math.isnan(s["mean_length"][1])
    ch = s["channels"]["reward_f32"]
    assert (ch["mean"][0], ch["std"][0], ch["min"][0], ch["max"][0]) == (5.0, 2.0, 3.0, 7.0)
    assert all(math.isnan(ch[k][1]) for k in ch)
    assert column_index("latency_ratio") == 17 and column_index("run_dur") == 5 and column_index("send rate") == 7 and column_index(6) == 6
    for bad in ("nope", 19, -1):
        with pytest.raises(ValueError):
            column_index(bad)


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_three_symbols_are_exported():
    L = lib()
    for s, n_args in EP_SYMBOLS.items():
        assert s in native.SYMBOLS, s
        assert hasattr(L, s), s
        assert len(getattr(L, s).argtypes) == n_args, s


def test_scratch_size():
    L = lib()
    for N, K, C, want in ((1, 1, 1, 6), (257, 1, 3, 2 * 14), (390, 6, 8, 6 * 34), (1024, 1024, 2, 1024 * 10), (65536, 8, 6, 8 * 32 * 26)):
        assert L.pcc_episode_scratch_doubles(N, K, C) == want, (N, K, C)
    for N, K, C in ((0, 1, 1), (-4, 1, 1), (8, 0, 1), (2050, 1025, 1), (9, 2, 1), (8, 1, 0), (8, 1, 9), (8, 1, -1)):
        assert L.pcc_episode_scratch_doubles(N, K, C) == -1, (N, K, C)


def test_refusals_need_no_device():
    """Everything outside the domain, and every NULL, returns -1 before any device call: the pointers here point nowhere."""
    L = lib()
    p = ctypes.c_void_p(4096)   # stands for a device pointer
    good_cols = (ctypes.c_int32 * 7)(6, 0, 1, 2, 5, 17, 18)

    def cols_of(*v):
        return (ctypes.c_int32 * len(v))(*v)

    def pop(reward=p, done=p, steps=p, cols=good_cols, C=3, T=4, N=12, K=3, carry=p, carry_len=p, last=p, last_len=p, totals=p,
            stride=None, scratch=p):
        return L.pcc_episode_update_pop(reward, done, steps, cols, C, T, N, K, carry, carry_len, last, last_len, totals,
                                        2 + 4 * C if stride is None else stride, scratch, None)

    def alone(reward=p, done=p, steps=p, cols=good_cols, C=3, T=4, N=12, K=1, carry=p, carry_len=p, last=p, last_len=p, totals=p,
              stride=None, scratch=p):
        assert K == 1
        return L.pcc_episode_update(reward, done, steps, cols, C, T, N, carry, carry_len, last, last_len, totals,
                                    2 + 4 * C if stride is None else stride, scratch, None)

    common = ({"C": 0}, {"C": 9}, {"C": -1}, {"T": 0}, {"T": -3}, {"N": 0}, {"N": -12}, {"stride": 13}, {"stride": 0},
              {"C": 8, "stride": 33}, {"reward": None}, {"done": None}, {"carry": None}, {"carry_len": None}, {"totals": None},
              {"scratch": None}, {"steps": None}, {"cols": None}, {"C": 2, "steps": None}, {"C": 2, "cols": None},
              {"cols": cols_of(6, 19)}, {"cols": cols_of(-1, 0)}, {"C": 8, "cols": cols_of(0, 1, 2, 3, 4, 5, 19)},
              {"C": 2, "cols": cols_of(1 << 20)})
    for call in (pop, alone):
        for kw in common:
            assert call(**kw) == -1, (call.__name__, kw)
    for kw in ({"K": 0}, {"K": -1}, {"K": 1025, "N": 2050}, {"N": 13}, {"K": 5}):
        assert pop(**kw) == -1, kw


def test_kernels_use_no_scratch(tmp_path):
    """A build into a temporary file: the two kernels -- one instantiation each, covering 8 channels -- are in the compiler's
    resource report with 0 bytes of scratch and 0 spilled vector registers; the unit is one of its own, and the figures the older
    tests pin for the policy kernels are still what the report says."""
    from pcc_rl_amd import build as pbuild
    assert "pcc_episodes.hip" in pbuild.UNITS
    out = str(tmp_path / "libpcc_sim_ep.so")
    pbuild.build_library(force=True, out=out)
    res = json.load(open(out + ".resources.json"))
    for name in ("episode_walk_kernel", "episode_merge_kernel"):
        assert name in res, name
        assert res[name]["scratch"] == 0 and res[name]["vgpr_spills"] == 0, (name, res[name])
        assert res[name]["lds"] <= 64 * 1024, (name, res[name])
    assert sorted(n for n in res if n.startswith("episode_")) == ["episode_merge_kernel", "episode_walk_kernel"]
    assert (res["ppo_grad_mfma_kernel<30, 32, 16>"]["vgprs"], res["ppo_grad_mfma_kernel<30, 32, 16>"]["lds"]) == (256, 52736)
    assert res["policy_act_fixed_kernel<30, 32, 16>"]["vgprs"] == 87
    assert (res["obs_moments_kernel"]["scratch"], res["obs_merge_kernel"]["scratch"]) == (0, 0)


# ------------------------------------------------------------------------------------------------------- the Python layer
def test_ledger_needs_a_gpu_device():
    with pytest.raises(ValueError, match="no CPU path"):
        EpisodeLedger(8, device="cpu")
    with pytest.raises(ValueError, match="do not divide"):
        EpisodeLedger(9, members=2, device="cuda:0")
    with pytest.raises(ValueError, match="at most 7"):
        EpisodeLedger(8, channels=range(8), device="cuda:0")
    with pytest.raises(ValueError, match="no step-record column"):
        EpisodeLedger(8, channels=("bogus",), device="cuda:0")


class _Env(object):
    """What PPO needs of an env, on the CPU, without a simulator behind it: 8 envs of 4 observations, episodes of 3 steps."""
    obs_dim, device, n_senders, n_envs = 4, "cpu", 1, 8

    def __init__(self):
        self.t = 0

    def reset(self):
        self.t = 0
        return torch.zeros((self.n_envs, self.obs_dim))

    def step(self, a):
        self.t += 1
        obs = torch.full((self.n_envs, self.obs_dim), float(self.t))
        return obs, -a.reshape(-1).abs(), torch.full((self.n_envs,), self.t % 3 == 0), {}

    def check_flags(self):
        pass

    def snapshot(self):
        return self.t


class _Env2(_Env):
    n_senders = 2


def test_without_the_option_the_keys_are_what_they_were():
    agent = PPO(_Env(), horizon=4, epochs=1, minibatch=16)
    assert agent.track_episodes is False and agent.ledger is None
    assert sorted(agent.iterate()) == ["entropy", "mean_step_reward", "pg", "vf"]
    assert sorted(agent.state_dict()) == ["device_rng", "env", "format", "fused_update", "n_envs", "obs", "obs_dim", "opt", "policy", "torch_rng"]


def test_constructors_refuse():
    with pytest.raises(ValueError, match="no CPU path"):
        PPO(_Env(), track_episodes=True)
    with pytest.raises(ValueError, match="one sender"):
        PPO(_Env2(), track_episodes=True)
    with pytest.raises(ValueError, match="BatchedNetworkEnv"):   # past the option: the argument checks as before
        PopulationPPO(_Env(), 2, track_episodes=True)


def test_a_checkpoint_without_the_option_is_refused_with_it():
    agent = PPO(_Env(), horizon=4, epochs=1, minibatch=16)
    sd = agent.state_dict()
    sd["track_episodes"] = True
    with pytest.raises(ValueError, match="track_episodes=True, this object has track_episodes=False"):
        agent.load_state_dict(sd)
