"""Closed-loop rollouts (pcc_rollout, BatchedNetworkEnv.rollout, PPO(policy_in_step=True)).

The contract (include/pcc_sim.h): the outputs are bit-identical to the loop "policy kernel on observation row t, then
pcc_step with that action".  Every GPU test runs that loop on a second handle with the same seed and compares every
output with torch.equal -- across the three routes of the library (the policy in the retire launch's epilogue, in the
small-batch kernel's loop, launch by launch) and the episode boundaries and restarts that decide between a stand-alone
policy launch and the epilogue.
"""
import ctypes

import numpy as np
import pytest
import torch

import pcc_rl_amd
from pcc_rl_amd import native
from pcc_rl_amd.native import PccError, lib

PCC_EINVAL = -1

DEV = "cuda"
COLS = native.PCC_STEP_COLS


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_rollout_refuses_null_and_zero_steps():
    L = lib()
    buf = (ctypes.c_float * 4)()
    rc = L.pcc_rollout(None, ctypes.cast(buf, ctypes.c_void_p), 32, 16, 4, None, ctypes.cast(buf, ctypes.c_void_p),
                       None, None, None, None, None, None, 1, None)
    assert rc == PCC_EINVAL
    assert b"pcc_rollout" in L.pcc_last_error()
    rc = L.pcc_rollout(None, ctypes.cast(buf, ctypes.c_void_p), 32, 16, 0, None, ctypes.cast(buf, ctypes.c_void_p),
                       None, None, None, None, None, None, 1, None)
    assert rc == PCC_EINVAL and b"n_steps" in L.pcc_last_error()


def test_ppo_policy_in_step_needs_the_gpu():
    from pcc_rl_amd.ppo import PPO

    class CpuEnv(object):
        device = torch.device("cpu")
        obs_dim, n_senders, n_envs = 30, 1, 4

    with pytest.raises(ValueError, match="policy_in_step"):
        PPO(CpuEnv(), policy_in_step=True)


# ----------------------------------------------------------------------------------------------------------------- GPU
def _params(D, arch=(32, 16), seed=0):
    from pcc_rl_amd.ppo import MlpPolicy
    torch.manual_seed(seed)
    pol = MlpPolicy(D, 1, arch)
    with torch.no_grad():
        pol.log_std.fill_(-0.7)   # (a spread of actions that moves the rates both ways)
    return pol.flat_params().to(DEV)


def _make(N, seed, epilogue=True, **kw):
    env = pcc_rl_amd.BatchedNetworkEnv(N, device=DEV, seed=seed, **kw)
    # PCC_TUNE_ROLLOUT_EPILOGUE: the policy in the retire launch's epilogue at full size (off by default: measured slower)
    native.check(env._L.pcc_set_tuning(env._h, native.TUNE["rollout_epilogue"], 1.0 if epilogue else 0.0))
    env.reset()
    return env


def _buffers(env, T):
    N, S, D = env.n_envs, env.n_senders, env.obs_dim
    f = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    return dict(obs=f(T + 1, N, S, D), act=f(T, N, S), logp=f(T, N, S), val=f(T, N, S), rew=f(T, N, S),
                done=torch.full((T, N), 7, dtype=torch.uint8, device=DEV), steps=f(T, N, S, COLS).double())


def _loop(env, params, arch, noise, b, T):
    """The contract's loop, literally: pcc_policy_act + pcc_step per step."""
    L = lib()
    N, S, D = env.n_envs, env.n_senders, env.obs_dim
    st = env._stream()
    for t in range(T):
        rc = L.pcc_policy_act(_p(b["obs"][t]), N * S, D, _p(params), arch[0], arch[1], _p(None if noise is None else noise[t]),
                              None, _p(b["act"][t]), _p(b["logp"][t]), _p(b["val"][t]), st)
        assert rc == 0
        native.check(L.pcc_step(env._h, _p(b["act"][t]), 0, _p(b["obs"][t + 1]), _p(b["rew"][t]), _p(b["done"][t]),
                                _p(b["steps"][t]), 1 if env.auto_reset else 0, st))


def _compare(make, T, arch=(32, 16), deterministic=False, setup=None, params_seed=1, split=None):
    """Two handles from make(); `setup(env)` brings each to the same state; then T steps by pcc_rollout (in chunks of
    `split` steps when given) against the loop."""
    a, r = make(), make()
    if setup:
        setup(a)
        setup(r)
    params = _params(a.obs_dim, arch, params_seed)
    noise = None if deterministic else torch.randn((T, a.n_envs, a.n_senders), device=DEV,
                                                    generator=torch.Generator(device=DEV).manual_seed(5))
    ba, br = _buffers(a, T), _buffers(r, T)
    ba["obs"][0].copy_(a._obs)
    br["obs"][0].copy_(r._obs)
    chunks = [(0, T)] if not split else [(t, min(t + split, T)) for t in range(0, T, split)]
    for lo, hi in chunks:
        a.rollout(params, None if noise is None else noise[lo:hi], ba["obs"][lo:hi + 1], ba["act"][lo:hi], ba["logp"][lo:hi],
                  ba["val"][lo:hi], ba["rew"][lo:hi], ba["done"][lo:hi], ba["steps"][lo:hi], arch=arch)
    _loop(r, params, arch, noise, br, T)
    torch.cuda.synchronize()
    a.check_flags()
    r.check_flags()
    for k in ("obs", "act", "logp", "val", "rew", "done", "steps"):
        assert torch.equal(ba[k], br[k]), k
    done = ba["done"].bool()
    a.close()
    r.close()
    return done


def _masked_reset(env):
    """Out of lockstep: a third of the envs start over after 7 steps."""
    N = env.n_envs
    for _ in range(7):
        env.step(torch.zeros(N, device=DEV))
    env.reset(torch.arange(N, device=DEV) % 3 == 0)


def _small_batches(monkeypatch):
    # the suite's fixture files every batch in work lists: the small-batch tests want the library's own threshold
    monkeypatch.setattr(pcc_rl_amd.BatchedNetworkEnv, "DEFAULT_LIST_MIN_ENVS", None)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_epilogue_65536():
    _compare(lambda: _make(65536, 3), 64)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_full_size_launch_by_launch_default():
    _compare(lambda: _make(20011, 2, epilogue=False, max_steps=40), 50, split=23)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_epilogue_odd_size_across_the_boundary():
    # 20 011 envs (list path, partitions with a ragged tail), lockstep auto-reset at every 40th step: a reset launch follows
    # the episode's last step and the action after it comes from a stand-alone policy launch; calls straddle the boundaries
    done = _compare(lambda: _make(20011, 4, max_steps=40), 100, split=37)
    assert done[39].all() and done[79].all() and not done[38].any()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_epilogue_out_of_lockstep_with_restarts():
    # masked reset first, then auto_reset: envs finish at different steps and restart inside the step (shadows with Philox)
    done = _compare(lambda: _make(20011, 6, max_steps=30), 70, setup=_masked_reset)
    assert done.any(0).all() and not done.all(1).any()


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("wide", [0.0, 1e9])
def test_rollout_epilogue_16_and_8_lane_groups(wide):
    # RETIRE_WIDE_PREDICT 0 + a grid with room: as many envs as fit retired (and given their policy) by 16 lanes; 1e9: all by 8
    def make():
        env = _make(20000, 9)
        native.check(env._L.pcc_set_tuning(env._h, native.TUNE["retire_wide_predict"], wide))
        native.check(env._L.pcc_set_tuning(env._h, native.TUNE["retire_grid_frac"], 1.0))
        return env
    _compare(make, 24)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_obs_length_36_and_deterministic():
    _compare(lambda: _make(16384, 10, history_len=3, features=list(pcc_rl_amd.METRIC_NAMES)), 20)
    _compare(lambda: _make(16384, 11), 20, deterministic=True)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_small_batch_config2_across_the_boundary(monkeypatch):
    _small_batches(monkeypatch)
    done = _compare(lambda: _make(4096, 12, link_params=(200.0, 0.03, 5.0, 0.0, 60.0)), 420, split=150)
    assert done[399].all() and not done[398].any()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_small_batch_1000_envs(monkeypatch):
    _small_batches(monkeypatch)
    _compare(lambda: _make(1000, 13, max_steps=30), 75)
    _compare(lambda: _make(1000, 14, max_steps=30, auto_reset=False), 20, deterministic=True)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_launch_by_launch_paths(monkeypatch):
    _compare(lambda: _make(3000, 15, n_senders=2), 20)
    _compare(lambda: _make(3000, 16, latency_noise=1.1), 20)
    _compare(lambda: _make(3000, 17), 20, arch=(8, 4))
    _small_batches(monkeypatch)
    _compare(lambda: _make(1000, 18, max_steps=10), 25, setup=_masked_reset)   # small batch out of lockstep


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_refuses_cwnd_mode_and_unknown_shapes():
    env = _make(256, 19, use_cwnd=True)
    b = _buffers(env, 2)
    with pytest.raises(PccError, match="congestion-window"):
        env.rollout(_params(env.obs_dim), None, b["obs"], None, None, None, None, None)
    env.close()
    env = _make(256, 20, history_len=7)   # 21 observations: no policy kernel
    b = _buffers(env, 2)
    with pytest.raises(PccError, match="observation length 21"):
        env.rollout(_params(env.obs_dim), None, b["obs"], None, None, None, None, None)
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_small_batch_matches_the_oracle(monkeypatch):
    """The small-batch loop tied to the C reference: the oracle fed the actions the rollout took reproduces every step."""
    import oracle
    _small_batches(monkeypatch)
    N, T, seed = 512, 50, 21
    env = pcc_rl_amd.BatchedNetworkEnv(N, device=DEV, seed=seed, auto_reset=False)
    env.reset()
    b = _buffers(env, T)
    b["obs"][0].copy_(env._obs)
    env.rollout(_params(env.obs_dim), torch.randn((T, N), device=DEV), b["obs"], b["act"], None, None, None, None, b["steps"])
    ref = oracle.run_batch(b["act"][:, :, 0].t().double().cpu().numpy(), rng_mode=oracle.RNG_PHILOX, seed=seed)
    assert np.array_equal(b["steps"][:, :, 0].transpose(0, 1).cpu().numpy(), ref["steps"])
    assert np.array_equal(b["obs"][1:, :, 0].transpose(0, 1).cpu().numpy(), ref["obs"].astype(np.float32))
    env.close()


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("grouped", [False, True])
def test_ppo_policy_in_step_collect_is_bit_identical(grouped):
    from pcc_rl_amd.ppo import PPO

    def run(in_step):
        env = (pcc_rl_amd.GroupedNetworkEnv(16384, 2, device=DEV, seed=31, max_steps=40) if grouped
               else pcc_rl_amd.BatchedNetworkEnv(16384, device=DEV, seed=31, max_steps=40))
        ppo = PPO(env, horizon=48, seed=3, policy_in_step=in_step)
        out = [ppo.collect() for _ in range(2)]
        torch.cuda.synchronize()
        env.close()
        return out

    for ra, rb in zip(run(True), run(False)):
        for x, y in zip(ra, rb):
            assert torch.equal(x, y)
