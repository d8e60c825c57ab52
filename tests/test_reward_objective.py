"""Reward objectives on the GPU (include/pcc_policy.h: pcc_reward_objective_pop; pcc_rl_amd.objective).
Synthetic step records go straight to the C ABI and are held, rewards and sums, bit for bit against the numpy restatement of
tests/models/reward_objective_model.py on shapes with a partial wavefront, a partial workgroup, two workgroups, and horizons around
the unrolled time loop; a member of a population against the stand-alone call on its columns.  Real rollouts: the reference
objective reproduces the env's own reward rows on every rollout path and leaves training as it is without the option; another
objective reaches the ledger, the reward normaliser, the advantage estimation and the checkpoint."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import reward_norm_model as norm_model  # noqa: E402
import reward_objective_model as model  # noqa: E402

import pcc_rl_amd  # noqa: E402
from pcc_rl_amd.evaluate import evaluate  # noqa: E402
from pcc_rl_amd.native import lib  # noqa: E402
from pcc_rl_amd.objective import TERMS, RewardObjective  # noqa: E402
from pcc_rl_amd.ppo import PPO, PopulationPPO  # noqa: E402

DEV = "cuda:0"
POOLS = (2, 8, 32)   # (fixed ring pools: the library's default depends on the free device memory, and a snapshot needs equal pools)
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------- the C ABI on synthetic records
UNROLL = 4                                      # csrc/pcc_objective.hip: kObjUnroll
HORIZONS = (1, UNROLL - 1, UNROLL, UNROLL + 1, 19)
ALL_SIX = (3.0, -700.0, -1500.0, -40.0, -0.25, 1.5)
WEIGHTS = {1: [model.DEFAULT], 3: [model.DEFAULT, ALL_SIX, (0.0, -500.0, 0.0, -3.0, 0.0, 2.5)]}


def _call_pop(steps, K, weights, sums=True):
    """pcc_reward_objective_pop on device records [T][N][19]; the outputs start as NaN: every element is written."""
    T, N, _ = steps.shape
    w = _dev(np.asarray(weights, dtype=np.float64).reshape(K, 6))
    out = torch.full((T, N), float("nan"), device=DEV)
    s = torch.full((K, 7), float("nan"), dtype=torch.float64, device=DEV) if sums else None
    need = lib().pcc_objective_scratch_doubles(T, N, K)
    assert need == K * -(-(N // K) // 256) * 7
    scratch = torch.full((need,), float("nan"), dtype=torch.float64, device=DEV)
    assert lib().pcc_reward_objective_pop(_p(steps), T, N, K, _p(w), _p(out), _p(s), _p(scratch), _stream()) == 0
    torch.cuda.synchronize()
    return out, s


def _call_alone(steps, weights):
    T, N, _ = steps.shape
    w = _dev(np.asarray(weights, dtype=np.float64).reshape(6))
    out = torch.full((T, N), float("nan"), device=DEV)
    s = torch.full((7,), float("nan"), dtype=torch.float64, device=DEV)
    scratch = torch.empty(lib().pcc_objective_scratch_doubles(T, N, 1), dtype=torch.float64, device=DEV)
    assert lib().pcc_reward_objective(_p(steps), T, N, _p(w), _p(out), _p(s), _p(scratch), _stream()) == 0
    torch.cuda.synchronize()
    return out, s


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n_m", [1, 63, 64, 65, 255, 256, 257, 331])
def test_rewards_and_sums_equal_the_model(n_m, K):
    N = K * n_m
    for T in HORIZONS:
        host = model.make_steps(T, N, 1000 * n_m + 10 * K + T)
        steps = _dev(host)
        weights = WEIGHTS[K]
        out, sums = _call_pop(steps, K, weights)
        want, want_sums = model.reward(host, weights, K), model.sums(host, weights, K)
        assert torch.equal(_bits(out), _bits(_dev(want))), (T, "rewards")
        assert torch.equal(_bits(sums), _bits(_dev(want_sums))), (T, "sums")
        again, sums_again = _call_pop(steps, K, weights)              # two runs: equal bits
        assert torch.equal(_bits(out), _bits(again)) and torch.equal(_bits(sums), _bits(sums_again)), T
        no_sums, _ = _call_pop(steps, K, weights, sums=False)          # sums == NULL: the rewards alone
        assert torch.equal(_bits(out), _bits(no_sums)), T
        for m in range(K):                                            # a member: the stand-alone call on its columns
            c = slice(m * n_m, (m + 1) * n_m)
            one, one_sums = _call_alone(steps[:, c].contiguous(), weights[m])
            assert torch.equal(_bits(out[:, c]), _bits(one)) and torch.equal(_bits(sums[m]), _bits(one_sums)), (T, m)


@pytest.mark.gpu
def test_default_weights_are_the_reward_column_and_zero_weights_skip():
    T, N = 7, 331
    host = model.make_steps(T, N, 5)
    _, acc, _ = model.terms(host, model.DEFAULT)
    host[..., model.COL_REWARD] = acc * model.REWARD_SCALE            # what the env writes there
    for c in model.TERM_COLS[3:]:
        host[..., c] = np.nan                                         # the columns the reference objective does not weigh
    steps = _dev(host)
    out, sums = _call_pop(steps, 1, [model.DEFAULT])
    assert torch.equal(_bits(out), _bits(steps[..., model.COL_REWARD].float())) and bool(torch.isfinite(sums).all())
    assert not sums[0, 3:6].any()                                     # a skipped term sums to 0
    weighed, _ = _call_pop(steps, 1, [(10.0, -1e3, -2e3, 0.0, 1.0, 0.0)])
    assert bool(torch.isnan(weighed).all())                           # weighed: it is read
    host[..., model.METRIC_COL0:] = np.nan
    zero, zero_sums = _call_pop(_dev(host), 1, [[0.0] * 6])           # no term at all: +0.0f, whatever the records hold
    assert not _bits(zero).any() and not _bits(zero_sums).any()


@pytest.mark.gpu
def test_the_python_class_is_the_call():
    T, N, K = 5, 3 * 65, 3
    host = model.make_steps(T, N, 9)
    obj = RewardObjective(N, K, [{"throughput": 3, "loss": -1500}, RewardObjective.DEFAULT, ALL_SIX], device=DEV)
    rows = [[3.0, 0.0, -1500.0, 0.0, 0.0, 0.0], list(model.DEFAULT), list(ALL_SIX)]
    assert obj.rows == rows and not obj.uniform()
    out = obj.apply(_dev(host))
    assert torch.equal(_bits(out), _bits(_dev(model.reward(host, rows, K))))
    want_sums = model.sums(host, rows, K)
    assert torch.equal(_bits(obj.sums), _bits(_dev(want_sums)))
    rep = obj.report()
    n = T * 65
    assert rep["reward"] == [s / n for s in want_sums[:, 6].tolist()]
    assert sorted(rep["terms"][0]) == ["loss", "throughput"] and sorted(rep["terms"][2]) == sorted(TERMS)
    assert rep["terms"][1]["latency"] == want_sums[1, 1] / n
    into = torch.empty((T, N), device=DEV)
    assert obj.apply(_dev(host).reshape(T, N, 1, 19), out=into) is into and torch.equal(_bits(into), _bits(out))
    other = RewardObjective(N, K, device=DEV)
    assert other.uniform() and other.rows == [list(model.DEFAULT)] * 3
    other.load_state_dict(obj.state_dict())
    assert other.rows == rows and torch.equal(other.weights, obj.weights)
    with pytest.raises(ValueError, match="another shape"):
        RewardObjective(N, 1, device=DEV).load_state_dict(obj.state_dict())
    with pytest.raises(ValueError, match="step records"):
        obj.apply(_dev(host)[:, :-1].contiguous())


# ------------------------------------------------------------------------------------------------------------ real rollouts
N_ENVS, HORIZON, MAX_STEPS = 256, 20, 8        # dones on rows 7 and 15 of the first rollout, 3, 11 and 19 of the second
OTHER = {"throughput": 5.0, "latency": -2e3, "latency_ratio": -0.5}
OTHER_ROW = [5.0, -2e3, 0.0, 0.0, -0.5, 0.0]


def _env(seed, n=N_ENVS, **kw):
    return pcc_rl_amd.BatchedNetworkEnv(n, device=DEV, seed=seed, ring_pools=POOLS, max_steps=MAX_STEPS, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["plain", "policy_in_step", "grouped", "grouped_policy_in_step", "framework"])
def test_the_reference_objective_is_the_envs_reward(path):
    if path.startswith("grouped"):
        env = pcc_rl_amd.GroupedNetworkEnv(N_ENVS, 2, device=DEV, seed=21, ring_pools=POOLS, max_steps=MAX_STEPS)
    else:
        env = _env(21)
    arch = (32, 16, 8) if path == "framework" else (32, 16)             # three hidden layers: no pcc_policy_act, the torch module
    agent = PPO(env, arch=arch, horizon=HORIZON, seed=2, objective=RewardObjective.DEFAULT, policy_in_step=path.endswith("policy_in_step"),
                fused_update=path != "framework")
    for _ in range(2):
        rows = agent.collect()
        torch.cuda.synchronize()
        rew = rows[5]
        assert rew.data_ptr() != agent.env_rew_b.data_ptr() and bool(agent.done_b.any())
        assert torch.equal(_bits(rew), _bits(agent.env_rew_b))
        assert torch.equal(_bits(rew), _bits(agent.steps_b[..., model.COL_REWARD].float()))
        assert rew.unique().numel() > rew.numel() // 2
    env.close()


def _two_iterations(agent):
    stats = [agent.iterate() for _ in range(2)]
    torch.cuda.synchronize()
    return stats


@pytest.mark.gpu
@pytest.mark.parametrize("trainer", ["ppo", "population"])
def test_the_reference_objective_leaves_training_as_it_is(trainer):
    got = []
    for objective in (None, RewardObjective.DEFAULT):
        env = _env(22)
        if trainer == "ppo":
            agent = PPO(env, horizon=HORIZON, seed=3, rng="philox", objective=objective)
        else:
            agent = PopulationPPO(env, 4, horizon=HORIZON, seeds=[3, 4, 5, 6], gamma=[0.99, 0.9, 0.95, 0.8], rng="philox", objective=objective)
        stats = _two_iterations(agent)
        assert ("objective_terms" in stats[-1]) == (objective is not None)
        got.append((agent.flat.clone(), agent.adam_m.clone(), agent.obs.clone(), stats[-1]["mean_step_reward"]))
        if objective is None:
            assert agent.objective is None and agent.env_rew_b is None and agent.steps_b is None
            assert "objective" not in agent.state_dict()
        env.close()
    for a, b in zip(got[0][:3], got[1][:3]):
        assert torch.equal(_bits(a), _bits(b))
    assert got[0][3] == got[1][3]


@pytest.mark.gpu
def test_another_objective_is_what_the_learner_sees():
    env = _env(23)
    agent = PPO(env, horizon=HORIZON, seed=4, objective=OTHER, track_episodes=True, normalize_reward=True)
    assert agent.objective.rows == [OTHER_ROW] and agent.ledger.names == ["reward_f32", "reward"]
    rews, dones = [], []
    for it in range(2):
        stats = agent.iterate()
        torch.cuda.synchronize()
        steps = agent.steps_b.cpu().numpy()
        want = model.reward(steps, OTHER_ROW)
        got = agent.objective.apply(agent.steps_b)                       # (the rows of this rollout again: the call is a pure function)
        assert torch.equal(_bits(got), _bits(_dev(want)))
        assert not torch.equal(got, agent.env_rew_b)                     # the objective changes the rewards
        assert torch.equal(_bits(agent.env_rew_b), _bits(agent.steps_b[..., model.COL_REWARD].float()))
        rews.append(want)
        dones.append(agent.done_b.cpu().numpy())
        n = HORIZON * N_ENVS
        want_sums = model.sums(steps, OTHER_ROW)
        assert stats["objective_terms"] == {name: want_sums[0, k] / n for k, name in enumerate(TERMS) if OTHER_ROW[k] != 0.0}
        assert stats["mean_step_reward"] == float(_dev(want).mean())
    env.check_flags()
    # the ledger: channel 0 is the per-episode sum of the objective's rows, channel "reward" the env's own last_return
    rew, done = np.concatenate(rews), np.concatenate(dones)
    run, last = np.zeros(N_ENVS), np.zeros(N_ENVS)
    for t in range(rew.shape[0]):
        run = run + rew[t].astype(np.float64)
        last = np.where(done[t] != 0, run, last)
        run = np.where(done[t] != 0, 0.0, run)
    assert done.sum() == 5 * N_ENVS
    assert torch.equal(_bits(agent.ledger.last[:, 0].contiguous()), _bits(_dev(last)))
    assert torch.equal(agent.ledger.last[:, 1], env.episode_returns())
    assert not torch.equal(agent.ledger.last[:, 0], agent.ledger.last[:, 1])
    # the reward normaliser's running returns: the model's walk over the objective's rows
    _, carry = norm_model.walk(rew, done, [agent.gamma], np.zeros(N_ENVS))
    assert torch.equal(_bits(agent.rew_norm.ret_carry), _bits(_dev(carry)))
    env.close()


@pytest.mark.gpu
def test_collect_returns_the_objectives_rows_and_gae_reads_them():
    env = _env(24)
    agent = PPO(env, horizon=HORIZON, seed=5, objective=OTHER)
    obs_b, act_b, logp_b, adv, ret, rew = agent.collect()
    torch.cuda.synchronize()
    want = _dev(model.reward(agent.steps_b.cpu().numpy(), OTHER_ROW))
    assert torch.equal(_bits(rew), _bits(want)) and not torch.equal(rew, agent.env_rew_b)
    from pcc_rl_amd.ppo import gae_fused
    with torch.no_grad():
        last_v = agent.policy.value(agent.obs)
    adv_want, _ = gae_fused(want, agent.val_b, agent.done_b, last_v, agent.gamma, agent.lam)
    adv_env, _ = gae_fused(agent.env_rew_b, agent.val_b, agent.done_b, last_v, agent.gamma, agent.lam)
    assert torch.equal(_bits(adv), _bits(adv_want)) and not torch.equal(adv, adv_env)
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
    want_rows = [t.clone() for t in (a.env_rew_b, a.steps_b, a.objective.sums)]
    env.close()
    env2, b = make()
    b.iterate()                                                          # (another state: everything comes from the checkpoint)
    b.load_state_dict(sd)
    for _ in range(2):
        b.iterate()
    torch.cuda.synchronize()
    for n in names:
        assert torch.equal(_bits(getattr(b, n)), _bits(want[n])), n
    for x, y in zip(want_rows, (b.env_rew_b, b.steps_b, b.objective.sums)):
        assert torch.equal(_bits(x), _bits(y))
    return env2, b, sd


@pytest.mark.gpu
def test_ppo_resume_is_bit_for_bit():
    def make():
        env = _env(25)
        return env, PPO(env, horizon=HORIZON, seed=6, objective=OTHER)

    env, agent, sd = _resume(make)
    env.close()
    env = _env(25)
    plain = PPO(env, horizon=HORIZON, seed=6)
    assert sd["objective"] is True and sorted(set(sd) - set(plain.state_dict())) == ["objective", "objective_state"]
    assert sd["objective_state"]["weights"].tolist() == [OTHER_ROW]
    with pytest.raises(ValueError, match="written with objective="):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="written with objective="):
        agent.load_state_dict(plain.state_dict())
    env.close()


PER_MEMBER = [RewardObjective.DEFAULT, OTHER, {"throughput": 10.0, "loss": -4e3}, ALL_SIX]


@pytest.mark.gpu
def test_population_resume_is_bit_for_bit_and_the_weights_stay_with_their_slots():
    def make():
        env = _env(26)
        return env, PopulationPPO(env, 4, horizon=HORIZON, seeds=[5, 6, 7, 8], gamma=[0.99, 0.9, 0.95, 0.8], objective=PER_MEMBER,
                                  track_episodes=True)

    env, pop, sd = _resume(make)
    rows = [list(model.DEFAULT), OTHER_ROW, [10.0, 0.0, -4e3, 0.0, 0.0, 0.0], list(ALL_SIX)]
    assert pop.objective.rows == rows and sd["objective_state"]["weights"].tolist() == rows
    n_m = N_ENVS // 4
    steps = pop.steps_b.cpu().numpy()
    rew = pop.objective.apply(pop.steps_b)
    assert torch.equal(_bits(rew), _bits(_dev(model.reward(steps, rows, 4))))          # every member its own objective
    assert torch.equal(_bits(rew[:, :n_m]), _bits(pop.env_rew_b[:, :n_m]))             # member 0: the reference
    assert not torch.equal(rew[:, n_m:], pop.env_rew_b[:, n_m:])
    stats = pop.iterate()
    assert [sorted(t) for t in stats["objective_terms"]] == [sorted(n for n, w in zip(TERMS, r) if w != 0.0) for r in rows]
    with pytest.raises(ValueError, match="different objectives do not rank"):
        pop.evolve()
    weights = pop.objective.weights.clone()
    flat = pop.flat.clone()
    parent, _ = pop.evolve(scores=[3.0, 0.0, 2.0, 1.0], frac=0.25)
    assert parent.tolist() == [0, 0, 2, 3] and torch.equal(pop.flat[1], flat[0])         # member 1 takes member 0's parameters ...
    assert torch.equal(_bits(pop.objective.weights), _bits(weights)) and pop.objective.rows == rows   # ... and keeps its objective
    pop.iterate()
    torch.cuda.synchronize()
    assert torch.equal(_bits(pop.objective.apply(pop.steps_b)), _bits(_dev(model.reward(pop.steps_b.cpu().numpy(), rows, 4))))
    env.close()
    env = _env(26)
    plain = PopulationPPO(env, 4, horizon=HORIZON, track_episodes=True)
    assert "objective" not in plain.state_dict() and "objective_state" not in plain.state_dict()
    with pytest.raises(ValueError, match="written with objective="):
        plain.load_state_dict(sd)
    env.close()


@pytest.mark.gpu
def test_evaluate_feeds_the_ledger_the_objectives_rows():
    N = 64
    out = {}
    for name, objective in (("none", None), ("default", RewardObjective.DEFAULT), ("other", OTHER)):
        env = _env(27, n=N)
        out[name] = evaluate(env, lambda obs, act: act.zero_(), episodes=2, channels=("reward",), objective=objective)
        out[name]["last"] = out[name]["last"].clone()
        env.close()
    ch = lambda r, c: r["channels"][c]["mean"][0]
    assert torch.equal(_bits(out["none"]["last"]), _bits(out["default"]["last"]))
    assert torch.equal(out["none"]["last"][:, 1], out["other"]["last"][:, 1]) and ch(out["none"], "reward") == ch(out["other"], "reward")
    assert not torch.equal(out["none"]["last"][:, 0], out["other"]["last"][:, 0])
    assert ch(out["none"], "reward_f32") == ch(out["default"], "reward_f32") != ch(out["other"], "reward_f32")


@pytest.mark.gpu
def test_two_senders_are_refused():
    env = pcc_rl_amd.BatchedNetworkEnv(8, device=DEV, seed=1, n_senders=2, ring_pools=POOLS)
    with pytest.raises(ValueError, match="objective=.*one sender"):
        PPO(env, objective=RewardObjective.DEFAULT)
    env.close()
