"""Time-limit bootstrapping on the GPU (include/pcc_policy.h: pcc_terminal_obs, pcc_gae_boot, pcc_gae_boot_pop;
pcc_rl_amd.timelimit; PPO / PopulationPPO with bootstrap_time_limit=True).

Everything is exact.  The rebuilt terminal observations are held against the env itself: a twin handle with the same seed, driven by
the same action rows with auto_reset=False, shows after the step that sets done the observation the first handle overwrote.  Slots,
zero rows and counts, and the bootstrapped advantage estimation, are held bit for bit against the numpy restatements of
tests/models/time_limit_model.py; a member against the stand-alone call on a copy of its columns; rows without a done against
pcc_gae.  Shapes: 200 envs leave a partial last wavefront (8 lanes: the copy hit by hit) behind three full ones (the copy as one run
in lockstep, hit by hit out of it); H F = 3, 30, 36 and, more than a wavefront's 64 lanes, 120."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import time_limit_model as model  # noqa: E402

import pcc_rl_amd  # noqa: E402
from pcc_rl_amd import timelimit  # noqa: E402
from pcc_rl_amd.metrics import METRIC_NAMES  # noqa: E402
from pcc_rl_amd.native import lib  # noqa: E402
from pcc_rl_amd.obsnorm import ObsNormalizer  # noqa: E402
from pcc_rl_amd.ppo import PPO, MlpPolicy, PopulationPPO, gae  # noqa: E402

DEV = "cuda:0"
POOLS = (2, 8, 32)   # (fixed ring pools: the library's default depends on the free device memory, and a snapshot needs equal pools)
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------- terminal rows against the env
N_TERM = 200
FEATURES = {"default-h10": (10, None), "all12-h3": (3, list(METRIC_NAMES)), "default-h1": (1, None), "all12-h10": (10, list(METRIC_NAMES))}


def _handle(n, auto_reset, max_steps, H=10, features=None, seed=11):
    return pcc_rl_amd.BatchedNetworkEnv(n, device=DEV, seed=seed, history_len=H, features=features, auto_reset=auto_reset,
                                        max_steps=max_steps, ring_pools=POOLS)


def _buffers(env, T):
    N, D = env.n_envs, env.obs_dim
    return (torch.full((T + 1, N, D), float("nan"), device=DEV), torch.full((T, N, 19), float("nan"), dtype=torch.float64, device=DEV),
            torch.full((T, N), 7, dtype=torch.uint8, device=DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("driver", ["rollout", "step_many"])
@pytest.mark.parametrize("shape", sorted(FEATURES))
def test_terminal_rows_are_the_twins_observations(shape, driver):
    """max_steps = T = 6: every env's first done is on the last row.  The twin (auto_reset=False) keeps the observation the first
    handle replaced with the next episode's first one."""
    H, features = FEATURES[shape]
    T = 6
    env, twin = _handle(N_TERM, True, T, H, features), _handle(N_TERM, False, T, H, features)
    N, D = env.n_envs, env.obs_dim
    obs_b, steps_b, done_b = _buffers(env, T)
    obs_b[0] = env.reset()
    first = twin.reset().clone()
    assert torch.equal(obs_b[0], first)
    torch.manual_seed(3)
    if driver == "rollout":
        arch = (32, 16) if D in (3, 6, 12, 30, 36, 60) else (16, 8)       # (pcc_rollout's 32,16 kernel has these lengths)
        params = MlpPolicy(D, 1, arch).to(DEV).flat_params()
        act_b = torch.empty((T, N, 1), device=DEV)
        env.rollout(params, torch.randn((T, N), device=DEV), obs_b, act_b, None, None, None, done_b, steps_b=steps_b, arch=arch)
    else:
        act_b = torch.rand((T, N, 1), device=DEV) * 2 - 1
        env.step_many(act_b, obs_out=obs_b[1:], done_out=done_b, steps_out=steps_b)
    twin_obs = torch.empty((T, N, D), device=DEV)
    twin_done = torch.empty((T, N), dtype=torch.uint8, device=DEV)
    twin.step_many(act_b, obs_out=twin_obs, done_out=twin_done)
    term_obs, term_count = timelimit.terminal_observations(env, obs_b, steps_b, done_b)
    torch.cuda.synchronize()
    env.check_flags(); twin.check_flags()
    assert torch.equal(done_b, twin_done) and not done_b[:T - 1].any() and done_b[T - 1].all()
    assert torch.equal(obs_b[1:T], twin_obs[:T - 1])                     # the same episode up to its end ...
    assert not torch.equal(obs_b[T], twin_obs[T - 1])                    # ... where the first handle shows the next one's start
    assert term_obs.shape == (1, N, D) and (term_count == 1).all()
    assert torch.equal(_bits(term_obs[0]), _bits(twin_obs[T - 1]))      # every env, every entry
    assert torch.isfinite(term_obs).all() and term_obs[0].abs().sum(1).min() > 0
    env.close(); twin.close()


@pytest.fixture(scope="module")
def staggered_rows():
    """200 envs out of lockstep, max_steps = 5, 17 recorded rows (computed once, left unchanged).  Before the recording the envs with
    i % 3 == 2 are set back by one step, so the others are done on row 0 and they on row 16; after row 2 the envs with i % 3 == 0 are
    reset (a masked reset): dones on rows 0, 7, 12 for them, 0, 5, 10, 15 and 1, 6, 11, 16 for the others."""
    T, N, S = 17, N_TERM, 5
    env = _handle(N, True, S)
    D = env.obs_dim
    idx = torch.arange(N, device=DEV)
    torch.manual_seed(4)

    def many(n, obs_out=None, **kw):
        env.step_many(torch.rand((n, N, 1), device=DEV) * 2 - 1, obs_out=obs_out, **kw)

    def masked_reset(mask, row):
        """The env's reset of the masked envs; `row`: the batch's observation row, the masked envs' entries replaced."""
        o = env.reset(mask).clone()
        row[mask] = o[mask]

    cur = torch.empty((3, N, D), device=DEV)
    cur[0] = env.reset()
    many(1, cur[:1])
    masked_reset(idx % 3 == 2, cur[0])
    many(3, cur)
    obs_b, steps_b, done_b = _buffers(env, T)
    obs_b[0] = cur[2]
    many(3, obs_b[1:4], done_out=done_b[:3], steps_out=steps_b[:3])
    masked_reset(idx % 3 == 0, obs_b[3])
    many(T - 3, obs_b[4:], done_out=done_b[3:], steps_out=steps_b[3:])
    torch.cuda.synchronize()
    env.check_flags()
    got = {"env": env, "obs": obs_b, "steps": steps_b, "done": done_b, "T": T, "N": N, "F": 3,
           "np": (obs_b.cpu().numpy(), steps_b.cpu().numpy(), done_b.cpu().numpy())}
    yield got
    env.close()


@pytest.mark.gpu
def test_slots_zero_rows_and_counts_out_of_lockstep(staggered_rows):
    r = staggered_rows
    env, T, N = r["env"], r["T"], r["N"]
    obs, steps, done = r["np"]
    assert done[0].any() and done[T - 1].any()                            # a done on the first row and one on the last
    times = {m: [t for t in range(T) if done[t, m]] for m in range(3)}
    assert times == {0: [0, 7, 12], 1: [0, 5, 10, 15], 2: [1, 6, 11, 16]}
    assert timelimit.slots(T, env.max_steps) == 4
    cols, scales = model.feature_columns(env.feature_ids)
    want_obs, want_count = model.terminal_obs(obs, steps, done, r["F"], cols, scales, 4)
    assert want_count.tolist() == [(3, 4, 4)[i % 3] for i in range(N)]
    out = (torch.full((4, N, env.obs_dim), float("nan"), device=DEV), torch.full((N,), -1, dtype=torch.int32, device=DEV))
    term_obs, term_count = timelimit.terminal_observations(env, r["obs"], r["steps"], r["done"], out=out)   # n_slots: the bound
    torch.cuda.synchronize()
    assert torch.equal(_bits(term_obs), _bits(_dev(want_obs))) and torch.equal(term_count, _dev(want_count))
    assert not term_obs[3, 0::3].any() and term_obs[3, 1::3].abs().sum(1).min() > 0                          # zero rows: never NaN
    # one slot on the same rows: the first done alone, the counts as they were
    one_obs, one_count = timelimit.terminal_observations(env, r["obs"], r["steps"], r["done"], n_slots=1)
    torch.cuda.synchronize()
    assert one_obs.shape == (1, N, env.obs_dim)
    assert torch.equal(_bits(one_obs[0]), _bits(_dev(want_obs[0]))) and torch.equal(one_count, _dev(want_count))
    # more slots than any env has dones: the rest are zeros
    six_obs, six_count = timelimit.terminal_observations(env, r["obs"], r["steps"], r["done"], n_slots=6)
    torch.cuda.synchronize()
    assert torch.equal(_bits(six_obs[:4]), _bits(_dev(want_obs))) and not six_obs[4:].any() and torch.equal(six_count, _dev(want_count))
    # the rows without the row T + 1 (what a caller with [T] observation rows passes): row T is not read
    cut_obs, _ = timelimit.terminal_observations(env, r["obs"][:T].contiguous(), r["steps"], r["done"])
    torch.cuda.synchronize()
    assert torch.equal(_bits(cut_obs), _bits(_dev(want_obs)))


# ------------------------------------------------------------------------------------------------------------ the advantages
GAE_SHAPES = [(1, 1), (17, 200), (64, 257)]
N_SLOTS = 2


def _gae_rows(T, N, K, dones=True):
    rng = np.random.default_rng(100 * T + N + K)
    rew = rng.standard_normal((T, N)).astype(np.float32)
    val = (rng.standard_normal((T, N)) * 3).astype(np.float32)
    last = rng.standard_normal(N).astype(np.float32)
    done = (rng.random((T, N)) < (0.15 if dones else 0.0)).astype(np.uint8)
    if dones and T > 2:
        done[1, 0] = done[2, 0] = 1                                       # two in adjacent rows
    if dones and T == 1:
        done[0, 0] = 1
    tv = rng.standard_normal((N_SLOTS, N)).astype(np.float32)
    tc = done.sum(0).astype(np.int32)
    gammas = np.linspace(0.99, 0.8, K).astype(np.float32)
    lams = np.linspace(0.95, 0.5, K).astype(np.float32)
    return rew, val, done, last, tv, tc, gammas, lams


def _hyper(gammas, lams):
    h = np.full((len(gammas), 8), 7.5, dtype=np.float32)                  # (the other columns hold what must not be read)
    h[:, 3], h[:, 4] = gammas, lams
    return _dev(h)


def _boot_pop(rew, val, done, last, tv, tc, hyper, K):
    T, N = rew.shape
    adv, ret = torch.full_like(rew, float("nan")), torch.full_like(rew, float("nan"))
    assert lib().pcc_gae_boot_pop(_p(rew), _p(val), _p(done), _p(last), _p(tv), _p(tc), tv.shape[0], T, N, K, _p(hyper), _p(adv), _p(ret),
                                  _stream()) == 0
    torch.cuda.synchronize()
    return adv, ret


def _boot(rew, val, done, last, tv, tc, gamma, lam):
    T, N = rew.shape
    adv, ret = torch.full_like(rew, float("nan")), torch.full_like(rew, float("nan"))
    assert lib().pcc_gae_boot(_p(rew), _p(val), _p(done), _p(last), _p(tv), _p(tc), tv.shape[0], T, N, float(gamma), float(lam), _p(adv),
                              _p(ret), _stream()) == 0
    torch.cuda.synchronize()
    return adv, ret


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("shape", GAE_SHAPES, ids=lambda s: "%d-%d" % s)
def test_gae_boot_equals_the_model(shape, K):
    T, N = shape[0], (shape[1] + K - 1) // K * K
    rew, val, done, last, tv, tc, gammas, lams = _gae_rows(T, N, K)
    assert T == 1 or (tc > N_SLOTS).any()                                 # a count above n_slots is among them
    want_adv, want_ret = model.gae_boot_members(rew, val, done, last, tv, tc, gammas, lams)
    d = [_dev(x) for x in (rew, val, done, last, tv, tc)]
    adv, ret = _boot_pop(*d, _hyper(gammas, lams), K)
    assert torch.equal(_bits(adv), _bits(_dev(want_adv))) and torch.equal(_bits(ret), _bits(_dev(want_ret)))
    # a member: the stand-alone call on a contiguous copy of its columns
    n_m = N // K
    for m in range(K):
        c = slice(m * n_m, (m + 1) * n_m)
        cols = [d[0][:, c].contiguous(), d[1][:, c].contiguous(), d[2][:, c].contiguous(), d[3][c].contiguous(), d[4][:, c].contiguous(),
                d[5][c].contiguous()]
        a1, r1 = _boot(*cols, gammas[m], lams[m])
        assert torch.equal(_bits(a1), _bits(adv[:, c])) and torch.equal(_bits(r1), _bits(ret[:, c])), m


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("shape", GAE_SHAPES, ids=lambda s: "%d-%d" % s)
def test_gae_boot_without_a_done_is_pcc_gae(shape, K):
    T, N = shape[0], (shape[1] + K - 1) // K * K
    rew, val, done, last, tv, tc, gammas, lams = _gae_rows(T, N, K, dones=False)
    assert not done.any() and not tc.any()
    d = [_dev(x) for x in (rew, val, done, last, tv, tc)]
    hyper = _hyper(gammas, lams)
    adv, ret = _boot_pop(*d, hyper, K)
    want_adv, want_ret = torch.empty_like(d[0]), torch.empty_like(d[0])
    assert lib().pcc_gae_pop(_p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), T, N, K, _p(hyper), _p(want_adv), _p(want_ret), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(adv), _bits(want_adv)) and torch.equal(_bits(ret), _bits(want_ret))
    if K == 1:
        a1, r1 = _boot(*d, gammas[0], lams[0])
        assert lib().pcc_gae(_p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), T, N, float(gammas[0]), float(lams[0]), _p(want_adv), _p(want_ret),
                             _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(a1), _bits(want_adv)) and torch.equal(_bits(r1), _bits(want_ret))


# ------------------------------------------------------------------------------------------------------------ the trainers
N_ENVS, HORIZON, MAX_STEPS = 256, 12, 8


def _env(seed, n=N_ENVS, max_steps=MAX_STEPS, **kw):
    return pcc_rl_amd.BatchedNetworkEnv(n, device=DEV, seed=seed, ring_pools=POOLS, max_steps=max_steps, **kw)


def _model_terminal(agent, raw_rows):
    """The model's terminal rows and counts of the agent's last rollout: raw_rows [T][N][D], the rows the env wrote."""
    cols, scales = model.feature_columns(agent.env.feature_ids)
    return model.terminal_obs(raw_rows.cpu().numpy(), agent.steps_b.cpu().numpy(), agent.done_b.cpu().numpy(), len(cols), cols, scales,
                              agent.time_limit.n_slots)


def _values(agent, params, rows):
    """pcc_policy_act's value output on every slot's rows [n_slots][N][D] under `params`."""
    h1, h2 = agent.policy.hidden
    out = torch.empty(rows.shape[:2], device=DEV)
    for k in range(rows.shape[0]):
        assert lib().pcc_policy_act(_p(rows[k]), rows.shape[1], rows.shape[2], _p(params), h1, h2, None, None, None, None, _p(out[k]),
                                    _stream()) == 0
    torch.cuda.synchronize()
    return out


def _want_adv(agent, term_val, term_count, rew):
    with torch.no_grad():
        last_v = agent.policy.value(agent.obs)
    return model.gae_boot(rew.cpu().numpy(), agent.val_b.cpu().numpy(), agent.done_b.cpu().numpy(), last_v.cpu().numpy(),
                          term_val.cpu().numpy(), term_count, agent.gamma, agent.lam)


@pytest.mark.gpu
def test_ppo_bootstraps_from_the_terminal_values():
    env, env0 = _env(41), _env(41)
    agent = PPO(env, horizon=HORIZON, seed=2, bootstrap_time_limit=True)
    plain = PPO(env0, horizon=HORIZON, seed=2)
    assert plain.time_limit is None and plain.steps_b is None and agent.time_limit.n_slots == 2
    for it in range(2):                                                   # dones on row 7, then on rows 3 and 11: both slots
        params = agent.policy.flat_params().clone()                      # the rollout's own parameters
        torch.manual_seed(100 + it)
        obs_b, act_b, logp_b, adv, ret, rew = agent.collect()
        torch.manual_seed(100 + it)
        obs0, act0, logp0, adv0, ret0, rew0 = plain.collect()
        for a, b in ((obs_b, obs0), (act_b, act0), (logp_b, logp0), (rew, rew0), (agent.val_b, plain.val_b), (agent.done_b, plain.done_b)):
            assert torch.equal(a, b)                                      # the rollout is what it is without the option
        done = agent.done_b
        assert done.sum(0).eq(it + 1).all()
        want_obs, want_count = _model_terminal(agent, obs_b)
        assert torch.equal(_bits(agent.time_limit.term_obs), _bits(_dev(want_obs)))
        assert torch.equal(agent.time_limit.term_count, _dev(want_count)) and agent.time_limit.term_in is agent.time_limit.term_obs
        term_val = _values(agent, params, _dev(want_obs))
        assert torch.equal(_bits(agent.time_limit.term_val), _bits(term_val))
        want_adv, want_ret = _want_adv(agent, term_val, want_count, rew)
        assert torch.equal(_bits(adv), _bits(_dev(want_adv))) and torch.equal(_bits(ret), _bits(_dev(want_ret)))
        # against the option-off agent: other numbers on exactly the samples at or before a done of their env in this rollout
        ends_in_done = done.flip(0).cummax(0).values.flip(0)
        assert ends_in_done.any() and ends_in_done.all() == (it == 1)       # (rows 0 .. 7; then, with a done on the last row, all)
        assert torch.equal(adv != adv0, ends_in_done) and torch.equal(ret != ret0, ends_in_done)
        assert torch.equal(_bits(adv[~ends_in_done]), _bits(adv0[~ends_in_done]))
        torch.manual_seed(200 + it)
        agent.update(obs_b, act_b, logp_b, adv0, ret0)                    # the same update for both: the next rollouts stay comparable
        torch.manual_seed(200 + it)
        plain.update(obs0, act0, logp0, adv0, ret0)
    s = agent.iterate()
    assert all(np.isfinite(v) for v in s.values()), s
    env.close(); env0.close()


@pytest.mark.gpu
def test_a_rollout_without_a_done_is_untouched():
    got = []
    for on in (False, True):
        env = _env(42, max_steps=400)
        agent = PPO(env, horizon=HORIZON, seed=3, bootstrap_time_limit=on)
        torch.manual_seed(7)
        rows = agent.collect()
        assert not agent.done_b.any()
        got.append([t.clone() for t in rows] + [agent.val_b.clone()])
        if on:
            assert agent.time_limit.n_slots == 1 and not agent.time_limit.term_count.any() and not agent.time_limit.term_obs.any()
        env.close()
    for a, b in zip(*got):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["policy_in_step", "grouped", "grouped_policy_in_step"])
def test_other_rollout_paths_give_the_same_bits(path):
    """With the policy inside the env's launches, over a GroupedNetworkEnv, and both, two iterations leave what the fused loop leaves."""
    got = []
    for other in (False, True):
        if other and path.startswith("grouped"):
            env = pcc_rl_amd.GroupedNetworkEnv(N_ENVS, 2, device=DEV, seed=43, ring_pools=POOLS, max_steps=MAX_STEPS)
        else:
            env = _env(43)
        agent = PPO(env, horizon=HORIZON, seed=3, bootstrap_time_limit=True, policy_in_step=other and path.endswith("policy_in_step"))
        torch.manual_seed(9)
        for _ in range(2):
            rows = agent.collect()
            agent.update(*rows[:5])
        torch.cuda.synchronize()
        tl = agent.time_limit
        assert agent.done_b.sum(0).eq(2).all()
        got.append([t.clone() for t in (rows[3], rows[4], agent.steps_b, tl.term_obs, tl.term_val, tl.term_count.float(), agent.flat)])
        env.close()
    for a, b, name in zip(got[0], got[1], ("adv", "ret", "steps", "term_obs", "term_val", "term_count", "weights")):
        assert torch.equal(_bits(a), _bits(b)), (path, name)


@pytest.mark.gpu
def test_ppo_framework_rollout_bootstraps_too():
    """fused_update=False and an --arch the policy kernel does not cover (three hidden layers): collect()'s framework branch, the
    torch module's values and ppo.gae(term_value=...)."""
    env = _env(44)
    agent = PPO(env, arch=(16, 16, 8), horizon=HORIZON, seed=2, bootstrap_time_limit=True, fused_update=False)
    for it in range(2):
        obs_b, act_b, logp_b, adv, ret, rew = agent.collect()
        want_obs, want_count = _model_terminal(agent, obs_b)
        assert want_count.tolist() == [it + 1] * N_ENVS
        assert torch.equal(_bits(agent.time_limit.term_obs), _bits(_dev(want_obs)))
        with torch.no_grad():
            term_val = torch.stack([agent.policy.value(r) for r in _dev(want_obs)])
            last_v = agent.policy.value(agent.obs)
        want_adv, want_ret = gae(rew, agent.val_b, agent.done_b, last_v, agent.gamma, agent.lam, term_val, _dev(want_count))
        assert torch.equal(_bits(adv), _bits(want_adv)) and torch.equal(_bits(ret), _bits(want_ret))
        plain_adv, _ = gae(rew, agent.val_b, agent.done_b, last_v, agent.gamma, agent.lam)
        assert not torch.equal(adv, plain_adv)
    env.close()


@pytest.mark.gpu
def test_normalised_observations_reach_the_value_network():
    """With normalize_obs the terminal rows are rebuilt from the raw rows and normalised with the statistics that were frozen for
    the rollout -- not the ones its end updates."""
    env = _env(45)
    agent = PPO(env, horizon=HORIZON, seed=2, bootstrap_time_limit=True, normalize_obs=True)
    for it in range(2):
        frozen = agent.obs_norm.norm.clone()
        params = agent.policy.flat_params().clone()
        obs_b, act_b, logp_b, adv, ret, rew = agent.collect()
        assert not torch.equal(frozen, agent.obs_norm.norm)               # (the rollout's end moved them)
        want_obs, want_count = _model_terminal(agent, agent.raw_b[:HORIZON])
        tl = agent.time_limit
        assert torch.equal(_bits(tl.term_obs), _bits(_dev(want_obs))) and tl.term_in is not tl.term_obs
        nz = ObsNormalizer(env.obs_dim, 1, agent.obs_norm.clip, agent.obs_norm.eps, device=DEV)
        nz.norm.copy_(frozen)
        want_in = torch.stack([nz.normalise(r) for r in _dev(want_obs)])
        assert torch.equal(_bits(tl.term_in), _bits(want_in))
        assert it == 0 or not torch.equal(want_in, _dev(want_obs))        # (once there are statistics the two differ)
        term_val = _values(agent, params, want_in)
        assert torch.equal(_bits(tl.term_val), _bits(term_val))
        want_adv, want_ret = _want_adv(agent, term_val, want_count, rew)
        assert torch.equal(_bits(adv), _bits(_dev(want_adv))) and torch.equal(_bits(ret), _bits(_dev(want_ret)))
        agent.update(obs_b, act_b, logp_b, adv, ret)
    env.close()


SEEDS, N_M = (4, 5, 6, 7), N_ENVS // 4


def _keep(agent, rows):
    K = getattr(agent, "members", 1)
    n_par = agent.n_params if isinstance(agent, PopulationPPO) else agent.flat.numel()
    flat = agent.flat.reshape(K, -1)[:, :n_par].clone()
    tl = agent.time_limit
    out = []
    for m in range(K):
        c = slice(m * N_M, (m + 1) * N_M)
        out.append({"flat": flat[m], "adv": rows[3][:, c].clone(), "ret": rows[4][:, c].clone(), "rew": rows[5][:, c].clone(),
                    "term_obs": tl.term_obs[:, c].clone(), "term_val": tl.term_val[:, c].clone(), "term_count": tl.term_count[c].clone()})
    return out


def _two_iterations(agent):
    for _ in range(2):
        rows = agent.collect()
        agent.update(*rows[:5])
    torch.cuda.synchronize()
    return rows


@pytest.mark.gpu
def test_a_member_equals_a_population_of_one():
    gammas, lams = [0.99, 0.9, 0.95, 0.8], [0.95, 0.9, 0.8, 0.99]
    env = _env(46)
    pop = PopulationPPO(env, 4, horizon=HORIZON, seeds=SEEDS, gamma=gammas, lam=lams, rng="philox", bootstrap_time_limit=True)
    whole = _keep(pop, _two_iterations(pop))
    assert pop.done_b.sum(0).eq(2).all() and pop.time_limit.term_val.abs().min() > 0
    env.close()
    for m, seed in enumerate(SEEDS):
        env = _env(46, n=N_M, env_gid_base=m * N_M)
        one = PopulationPPO(env, 1, horizon=HORIZON, seeds=[seed], gamma=gammas[m], lam=lams[m], rng="philox", bootstrap_time_limit=True)
        got = _keep(one, _two_iterations(one))[0]
        env.close()
        for k in got:
            assert torch.equal(_bits(whole[m][k].float()), _bits(got[k].float())), (m, k)
    # ... and the option changes the members' numbers
    env = _env(46)
    off = PopulationPPO(env, 4, horizon=HORIZON, seeds=SEEDS, gamma=gammas, lam=lams, rng="philox")
    rows = off.collect()
    assert off.time_limit is None
    env.close()
    env = _env(46)
    on = PopulationPPO(env, 4, horizon=HORIZON, seeds=SEEDS, gamma=gammas, lam=lams, rng="philox", bootstrap_time_limit=True)
    rows_on = on.collect()
    assert torch.equal(rows[5], rows_on[5]) and torch.equal(rows[0], rows_on[0])
    ends = on.done_b.flip(0).cummax(0).values.flip(0)
    assert torch.equal(rows[3] != rows_on[3], ends)
    env.close()


def _resume(make):
    names = ("flat", "adam_m", "adam_v", "obs")
    env, a = make()
    for _ in range(2):
        a.iterate()
    sd = a.state_dict()
    for _ in range(2):
        a.iterate()
    torch.cuda.synchronize()
    want = {n: getattr(a, n).clone() for n in names}
    want_tl = [t.clone() for t in (a.time_limit.term_obs, a.time_limit.term_val, a.steps_b)]
    env.close()
    env2, b = make()
    b.iterate()                                                          # (another state: everything comes from the checkpoint)
    b.load_state_dict(sd)
    for _ in range(2):
        b.iterate()
    torch.cuda.synchronize()
    for n in names:
        assert torch.equal(_bits(getattr(b, n)), _bits(want[n])), n
    for x, y in zip(want_tl, (b.time_limit.term_obs, b.time_limit.term_val, b.steps_b)):
        assert torch.equal(_bits(x), _bits(y))
    return env2, b, sd


@pytest.mark.gpu
def test_ppo_resume_is_bit_for_bit():
    def make():
        env = _env(47)
        return env, PPO(env, horizon=HORIZON, seed=4, bootstrap_time_limit=True)

    env, agent, sd = _resume(make)
    env.close()
    env = _env(47)
    plain = PPO(env, horizon=HORIZON, seed=4)
    assert sd["bootstrap_time_limit"] is True and sorted(set(sd) - set(plain.state_dict())) == ["bootstrap_time_limit"]   # no state
    with pytest.raises(ValueError, match="bootstrap_time_limit"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="bootstrap_time_limit"):
        agent.load_state_dict(plain.state_dict())
    env.close()


@pytest.mark.gpu
def test_population_resume_is_bit_for_bit():
    def make():
        env = _env(48)
        return env, PopulationPPO(env, 4, horizon=HORIZON, seeds=[5, 6, 7, 8], gamma=[0.99, 0.9, 0.95, 0.8], bootstrap_time_limit=True)

    env, pop, sd = _resume(make)
    env.close()
    env = _env(48)
    plain = PopulationPPO(env, 4, horizon=HORIZON)
    assert "bootstrap_time_limit" not in plain.state_dict()
    with pytest.raises(ValueError, match="bootstrap_time_limit"):
        plain.load_state_dict(sd)
    env.close()


@pytest.mark.gpu
def test_two_senders_are_refused():
    env = pcc_rl_amd.BatchedNetworkEnv(8, device=DEV, seed=1, n_senders=2, ring_pools=POOLS)
    with pytest.raises(ValueError, match="bootstrap_time_limit=True.*one sender"):
        PPO(env, bootstrap_time_limit=True)
    with pytest.raises(ValueError, match="one sender"):
        timelimit.terminal_observations(env, None, None, None)
    env.close()
