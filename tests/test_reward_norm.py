"""Reward normalisation on the GPU (include/pcc_policy.h: pcc_return_stats_update_pop, pcc_reward_normalise_pop and their
stand-alone forms; pcc_rl_amd.rewnorm.RewardNormalizer; PPO / PopulationPPO with normalize_reward=True).

The walk is exact: ret_carry is held bit for bit against the numpy restatement of tests/models/reward_norm_model.py.  The moments
are held against numpy's float64 two-pass mean and population variance of the model's samples: with n the member's sample count,
|mean - want| <= 8 n 2^-53 max|R| and |m2 / count - want| <= 8 n 2^-53 max|R|^2 (moment_bounds of tests/test_obs_norm_cpu.py: the
worst case of recursive summation, times 8 for the merge arithmetic).  Everything else is exact: the count, scale from the device's
own stats, the normalised rows, a member against the stand-alone call on a copy of its columns, a repeated call, the padding --
compared as int32 / int64 views.  Shapes (T, n_m, K): sample counts on both sides of the wavefront and workgroup edges, members
over several workgroups, and a whole episode's length in one call."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import reward_norm_model as model  # noqa: E402

import pcc_rl_amd  # noqa: E402
from pcc_rl_amd.native import lib  # noqa: E402
from pcc_rl_amd.ppo import PPO, PopulationPPO, gae_fused  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 1, 1), (5, 257, 3), (7, 4099, 2), (3, 65, 4), (3, 64, 1), (400, 64, 1)]
IDS = lambda s: "%d-%d-%d" % s
GAMMAS = (0.99, 0.0, 1.0, "each")   # "each": one different value per member
PAD, POISON = 2, -7777.25           # doubles behind every stats row, and what they hold
EPS = 1e-8
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _gammas(gamma, K):
    return np.linspace(0.5, 0.97, K).astype(np.float32) if gamma == "each" else model.member_gammas(gamma, K)


def _hyper(gammas):
    """The [K][8] block with gamma in column 3; the other columns hold what must not be read as gamma."""
    h = np.full((len(gammas), 8), 7.5, dtype=np.float32)
    h[:, 3] = gammas
    return torch.from_numpy(h).to(DEV)


def _fresh_stats(K):
    st = torch.zeros((K, 3 + PAD), dtype=torch.float64, device=DEV)
    st[:, 3:] = POISON
    return st


def _update(rew, done, K, gammas, carry, stats, scale=True, eps=EPS):
    """pcc_return_stats_update_pop on the device rows; returns scale (poisoned before the call)."""
    T, N = rew.shape
    need = lib().pcc_return_scratch_doubles(T, N, K)
    assert need > 0
    scratch = torch.full((need,), float("nan"), dtype=torch.float64, device=DEV)
    sc = torch.full((K,), float("nan"), device=DEV) if scale else None
    rc = lib().pcc_return_stats_update_pop(_p(rew), _p(done), T, N, K, _p(_hyper(gammas)), _p(carry), _p(stats), stats.stride(0), _p(sc),
                                           eps, _p(scratch), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return sc


def _update_alone(rew, done, gamma, carry, stats, eps=EPS):
    T, N = rew.shape
    scratch = torch.full((lib().pcc_return_scratch_doubles(T, N, 1),), float("nan"), dtype=torch.float64, device=DEV)
    sc = torch.full((1,), float("nan"), device=DEV)
    assert lib().pcc_return_stats_update(_p(rew), _p(done), T, N, float(gamma), _p(carry), _p(stats), _p(sc), eps, _p(scratch), _stream()) == 0
    torch.cuda.synchronize()
    return sc


def _check_moments(stats, samples, K, what):
    """Row m of stats against the float64 two-pass over member m's samples of every batch."""
    st = stats.cpu().numpy()
    assert (st[:, 3:] == POISON).all(), what                          # the padding is untouched
    for m in range(K):
        x = np.concatenate([model.member_samples(s, m, K) for s in samples])
        n, mean, m2 = model.batch_moments(x)
        b_mean, b_var = model.moment_bounds(n, float(np.abs(x).max()))
        assert st[m, 0] == n, (what, m)                               # the count is exact
        e_mean, e_var = abs(st[m, 1] - mean[0]), abs(st[m, 2] / n - m2[0] / n)
        assert e_mean <= b_mean, (what, m, e_mean, b_mean)
        assert e_var <= b_var, (what, m, e_var, b_var)
        assert st[m, 2] >= 0.0, (what, m)


def _check_scale(scale, stats, what):
    want = torch.from_numpy(model.scale_from_stats(stats.cpu().numpy(), EPS)).to(DEV)
    assert torch.equal(_bits(scale), _bits(want)), what


@pytest.mark.gpu
@pytest.mark.parametrize("kind", model.REWARD_KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_walk_and_moments_against_the_model(shape, kind):
    T, n_m, K = shape
    N = K * n_m
    rng = np.random.default_rng(T + n_m + K)
    for gamma in GAMMAS:
        gammas = _gammas(gamma, K)
        for done_kind in model.DONE_KINDS:
            what = (shape, kind, gamma, done_kind)
            r, d = model.make_rewards(kind, (T, N), rng), model.make_done(done_kind, (T, N), rng)
            rew, done = torch.from_numpy(r).to(DEV), torch.from_numpy(d).to(DEV)
            samples, carry_want = model.walk(r, d, gammas, np.zeros(N))
            carry, stats = torch.zeros(N, dtype=torch.float64, device=DEV), _fresh_stats(K)
            scale = _update(rew, done, K, gammas, carry, stats)
            assert np.array_equal(carry.cpu().numpy().view(np.int64), carry_want.view(np.int64)), what   # the walk, from a zero carry
            _check_moments(stats, [samples], K, what)
            _check_scale(scale, stats, what)
            # the same call on fresh state: the same bits; and scale == NULL writes the same stats
            carry2, stats2, carry3, stats3 = torch.zeros_like(carry), _fresh_stats(K), torch.zeros_like(carry), _fresh_stats(K)
            scale2 = _update(rew, done, K, gammas, carry2, stats2)
            assert _update(rew, done, K, gammas, carry3, stats3, scale=False) is None
            assert torch.equal(stats2, stats) and torch.equal(stats3, stats) and torch.equal(_bits(scale2), _bits(scale)), what
            assert torch.equal(_bits(carry2), _bits(carry)) and torch.equal(_bits(carry3), _bits(carry)), what
            # the walk from a non-zero carry
            start = rng.standard_normal(N) * 100.0
            _, carry_want = model.walk(r, d, gammas, start)
            carry = torch.from_numpy(start).to(DEV)
            _update(rew, done, K, gammas, carry, _fresh_stats(K))
            assert np.array_equal(carry.cpu().numpy().view(np.int64), carry_want.view(np.int64)), what


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_split_calls_leave_the_same_carry(shape):
    """[0, T) in one call and in two calls over [0, T1) and [T1, T): ret_carry bit for bit, the count exactly, the other moments
    within the bound of the same two-pass (T = 1 has no split: two rows there)."""
    T, n_m, K = shape
    T, N = max(T, 2), K * n_m
    rng = np.random.default_rng(2 * T + n_m)
    gammas = _gammas("each", K)
    for kind in model.REWARD_KINDS:
        r, d = model.make_rewards(kind, (T, N), rng), model.make_done("bernoulli", (T, N), rng)
        rew, done = torch.from_numpy(r).to(DEV), torch.from_numpy(d).to(DEV)
        start = rng.standard_normal(N) * 10.0
        samples, carry_want = model.walk(r, d, gammas, start)
        for T1 in sorted({1, T // 2, T - 1}):
            whole, parts = torch.from_numpy(start).to(DEV), torch.from_numpy(start).to(DEV)
            st_whole, st_parts = _fresh_stats(K), _fresh_stats(K)
            _update(rew, done, K, gammas, whole, st_whole)
            _update(rew[:T1].contiguous(), done[:T1].contiguous(), K, gammas, parts, st_parts)
            _update(rew[T1:].contiguous(), done[T1:].contiguous(), K, gammas, parts, st_parts)
            assert torch.equal(_bits(whole), _bits(parts)), (shape, kind, T1)
            assert np.array_equal(whole.cpu().numpy().view(np.int64), carry_want.view(np.int64)), (shape, kind, T1)
            assert torch.equal(st_whole[:, 0], st_parts[:, 0]), (shape, kind, T1)
            _check_moments(st_parts, [samples], K, (shape, kind, T1))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_three_updates_against_the_concatenation(shape):
    T, n_m, K = shape
    N = K * n_m
    rng = np.random.default_rng(n_m + 7 * T)
    gammas = _gammas("each", K)
    carry, stats = torch.zeros(N, dtype=torch.float64, device=DEV), _fresh_stats(K)
    carry_np, samples = np.zeros(N), []
    for i, kind in enumerate(model.REWARD_KINDS):                       # (other row counts, other kinds)
        r, d = model.make_rewards(kind, (T + i, N), rng), model.make_done("bernoulli", (T + i, N), rng)
        s, carry_np = model.walk(r, d, gammas, carry_np)
        samples.append(s)
        scale = _update(torch.from_numpy(r).to(DEV), torch.from_numpy(d).to(DEV), K, gammas, carry, stats)
        assert np.array_equal(carry.cpu().numpy().view(np.int64), carry_np.view(np.int64)), (shape, i)
        _check_moments(stats, samples, K, (shape, i))
        _check_scale(scale, stats, (shape, i))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_members_equal_stand_alone_calls(shape):
    """stats, scale, ret_carry and out of every member: bit-equal to the stand-alone entry points on a contiguous copy of its
    columns -- after one update and after a second one into the running row."""
    T, n_m, K = shape
    N = K * n_m
    rng = np.random.default_rng(3 * n_m + T)
    gammas = _gammas("each", K)
    carry, stats = torch.zeros(N, dtype=torch.float64, device=DEV), _fresh_stats(K)
    alone = [(torch.zeros(n_m, dtype=torch.float64, device=DEV), torch.zeros((1, 3), dtype=torch.float64, device=DEV)) for _ in range(K)]
    for kind in ("offset", "wide"):
        rew = torch.from_numpy(model.make_rewards(kind, (T, N), rng)).to(DEV)
        done = torch.from_numpy(model.make_done("bernoulli", (T, N), rng)).to(DEV)
        scale = _update(rew, done, K, gammas, carry, stats)
        out = torch.full_like(rew, float("nan"))
        assert lib().pcc_reward_normalise_pop(_p(rew), T, N, K, _p(scale), 2.5, _p(out), _stream()) == 0
        for m in range(K):
            cols = slice(m * n_m, (m + 1) * n_m)
            mine, mine_done = rew[:, cols].contiguous(), done[:, cols].contiguous()
            carry_m, stats_m = alone[m]
            scale_m = _update_alone(mine, mine_done, gammas[m], carry_m, stats_m)
            assert torch.equal(stats_m[0], stats[m, :3]), (shape, kind, m)
            assert torch.equal(_bits(scale_m[0]), _bits(scale[m])), (shape, kind, m)
            assert torch.equal(_bits(carry_m), _bits(carry[cols])), (shape, kind, m)
            out_m = torch.full_like(mine, float("nan"))
            assert lib().pcc_reward_normalise(_p(mine), T, n_m, _p(scale_m), 2.5, _p(out_m), _stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(_bits(out_m), _bits(out[:, cols])), (shape, kind, m)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_normalise_equals_the_restatement(shape):
    T, n_m, K = shape
    N = K * n_m
    rng = np.random.default_rng(n_m + T)
    x = model.make_rewards("wide", (T, N), rng)
    x.reshape(-1)[::5] *= np.float32(1e6)                              # far beyond the clip, both signs
    x.reshape(-1)[::11] = 0.0
    x.reshape(-1)[::13] = np.float32(3e38)                             # times a scale > 1: a product beyond float32
    x.reshape(-1)[::17] = np.nan                                       # fmaxf(NaN, -clip) = -clip
    x[T - 1, N - 1] = -3e38
    big = np.exp(rng.standard_normal(K) * 3.0).astype(np.float32) + np.float32(1.5)
    small = np.exp(rng.standard_normal(K) * 3.0 - 8.0).astype(np.float32)
    rew = torch.from_numpy(x).to(DEV)
    for scale_np, clip in ((big, 10.0), (small, 0.37), (np.ones(K, np.float32), 5.0)):
        want = model.normalise(x, scale_np, K, clip)
        assert not np.isnan(want).any()
        scale = torch.from_numpy(scale_np).to(DEV)
        out = torch.full_like(rew, float("nan"))
        assert lib().pcc_reward_normalise_pop(_p(rew), T, N, K, _p(scale), clip, _p(out), _stream()) == 0
        again = torch.full_like(rew, float("nan"))
        assert lib().pcc_reward_normalise_pop(_p(rew), T, N, K, _p(scale), clip, _p(again), _stream()) == 0
        inplace = rew.clone()                                          # out == reward
        assert lib().pcc_reward_normalise_pop(_p(inplace), T, N, K, _p(scale), clip, _p(inplace), _stream()) == 0
        torch.cuda.synchronize()
        w = _bits(torch.from_numpy(want).to(DEV))
        assert torch.equal(_bits(out), w) and torch.equal(_bits(again), w) and torch.equal(_bits(inplace), w), (shape, clip)
        # a view that starts 4 bytes off a 16-byte boundary: the float-by-float path gives the same bits
        off_in, off_out = torch.empty(T * N + 1, device=DEV), torch.full((T * N + 1,), float("nan"), device=DEV)
        off_in[1:] = rew.reshape(-1)
        assert lib().pcc_reward_normalise_pop(_p(off_in[1:]), T, N, K, _p(scale), clip, _p(off_out[1:]), _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(off_out[1:].reshape(T, N)), w), (shape, clip)
    assert torch.equal(_bits(rew), _bits(torch.from_numpy(x).to(DEV)))  # the input of the out-of-place calls is as it was


# ------------------------------------------------------------------------------------------------------------ the trainers
POOLS = (2, 8, 32)   # (fixed ring pools: the library's default depends on the free device memory, and a snapshot needs equal pools)
N_ENVS, HORIZON, CLIP = 256, 8, 10.0


def _env(seed, **kw):
    return pcc_rl_amd.BatchedNetworkEnv(N_ENVS, device=DEV, seed=seed, ring_pools=POOLS, **kw)


def _check_rollout(agent, rew, gammas, carry_before, samples_so_far, K=1):
    """After a collect(): the normaliser's state against the model fed with the returned raw rows, and rew_norm_b against the
    restatement with the device's own scale.  Returns the carry the model holds now."""
    r, d = rew.cpu().numpy(), agent.done_b.cpu().numpy()
    s, carry = model.walk(r, d, gammas, carry_before)
    samples_so_far.append(s)
    nz = agent.rew_norm
    assert np.array_equal(nz.ret_carry.cpu().numpy().view(np.int64), carry.view(np.int64))
    st = torch.cat([nz.stats, torch.full((K, PAD), POISON, dtype=torch.float64, device=DEV)], dim=1)
    _check_moments(st, samples_so_far, K, "trainer")
    _check_scale(nz.scale, nz.stats, "trainer")
    want = model.normalise(r, nz.scale.cpu().numpy(), K, CLIP)
    assert torch.equal(_bits(agent.rew_norm_b), _bits(torch.from_numpy(want).to(DEV)))
    return carry


@pytest.mark.gpu
def test_ppo_estimates_advantages_from_normalised_rewards():
    env, env0 = _env(31), _env(31)
    agent = PPO(env, horizon=HORIZON, seed=2, normalize_reward=True, clip_reward=CLIP)
    plain = PPO(env0, horizon=HORIZON, seed=2)
    assert plain.rew_norm is None and plain.rew_norm_b is None
    assert torch.equal(agent.rew_norm.scale, torch.ones(1, device=DEV)) and not agent.rew_norm.ret_carry.any()
    carry, samples = np.zeros(N_ENVS), []
    for it in range(2):
        torch.manual_seed(100 + it)
        obs_b, act_b, logp_b, adv, ret, rew = agent.collect()
        if it == 0:   # the sixth value is the raw rows: what the trainer without the option returns from the same env, seed and noise
            torch.manual_seed(100 + it)
            assert torch.equal(_bits(rew), _bits(plain.collect()[5]))
        assert rew.data_ptr() != agent.rew_norm_b.data_ptr() and not torch.equal(rew, agent.rew_norm_b)
        carry = _check_rollout(agent, rew, [agent.gamma], carry, samples)
        with torch.no_grad():
            last_v = agent.policy.value(agent.obs)
        adv_w, ret_w = gae_fused(agent.rew_norm_b, agent.val_b, agent.done_b, last_v, agent.gamma, agent.lam)
        assert torch.equal(_bits(adv), _bits(adv_w)) and torch.equal(_bits(ret), _bits(ret_w))
        adv_raw, _ = gae_fused(rew, agent.val_b, agent.done_b, last_v, agent.gamma, agent.lam)
        assert not torch.equal(adv, adv_raw)
        agent.update(obs_b, act_b, logp_b, adv, ret)
    s = agent.iterate()
    assert all(np.isfinite(v) for v in s.values()), s
    assert float(agent.rew_norm.stats[0, 0]) == 3 * HORIZON * N_ENVS
    env.close(); env0.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["policy_in_step", "grouped"])
def test_other_rollout_paths_give_the_same_bits(path):
    """The option acts after the rollout: with the policy inside the env's launches, and over a GroupedNetworkEnv after its streams
    joined, two iterations leave what the fused loop leaves, bit for bit."""
    got = []
    for other in (False, True):
        if other and path == "grouped":
            env = pcc_rl_amd.GroupedNetworkEnv(N_ENVS, 2, device=DEV, seed=32, ring_pools=POOLS)
        else:
            env = _env(32)
        agent = PPO(env, horizon=HORIZON, seed=3, normalize_reward=True, policy_in_step=other and path == "policy_in_step")
        for _ in range(2):
            agent.iterate()
        torch.cuda.synchronize()
        nz = agent.rew_norm
        got.append([t.clone() for t in (agent.rew_norm_b, nz.stats, nz.scale, nz.ret_carry, agent.flat)])
        env.close()
    for a, b, name in zip(got[0], got[1], ("rew_norm_b", "stats", "scale", "ret_carry", "weights")):
        assert torch.equal(_bits(a), _bits(b)), (path, name)
    assert float(got[0][1][0, 0]) == 2 * HORIZON * N_ENVS


@pytest.mark.gpu
def test_ppo_framework_rollout_normalises_too():
    """fused_update=False and an --arch the policy kernel does not cover (three hidden layers): collect()'s framework branch."""
    env = _env(33)
    agent = PPO(env, arch=(16, 16, 8), horizon=HORIZON, seed=2, normalize_reward=True, fused_update=False)
    carry, samples = np.zeros(N_ENVS), []
    for _ in range(2):
        rew = agent.collect()[5]
        carry = _check_rollout(agent, rew, [agent.gamma], carry, samples)
    env.close()


@pytest.mark.gpu
def test_population_members_keep_their_own_statistics_and_inherit_them():
    K = 4
    gammas = [0.99, 0.9, 0.95, 0.5]
    env = _env(34)
    pop = PopulationPPO(env, K, horizon=HORIZON, seeds=[1, 2, 3, 4], gamma=gammas, normalize_reward=True, clip_reward=CLIP)
    carry, samples = np.zeros(N_ENVS), []
    for _ in range(2):
        obs_b, act_b, logp_b, adv, ret, rew = pop.collect()
        carry = _check_rollout(pop, rew, np.array(gammas, dtype=np.float32), carry, samples, K)   # every member: its own gamma, its own columns
        adv_w, ret_w = pop._gae(pop.rew_norm_b, pop.val_b, pop.done_b, _last_values(pop))
        assert torch.equal(_bits(adv), _bits(adv_w)) and torch.equal(_bits(ret), _bits(ret_w))
        s = pop.update(obs_b, act_b, logp_b, adv, ret)
        assert all(np.isfinite(v).all() for v in s.values()), s
    nz = pop.rew_norm
    stats, scale, ret_carry = nz.stats.clone(), nz.scale.clone(), nz.ret_carry.clone()
    assert (stats[:, 0] == 2 * HORIZON * N_ENVS // K).all()
    for a in range(K):
        for b in range(a + 1, K):
            assert not torch.equal(stats[a], stats[b]) and not torch.equal(scale[a], scale[b]), (a, b)
    flat = pop.flat.clone()
    parent, _ = pop.evolve([3.0, 2.0, 1.0, 0.0], frac=0.5, seed=5)     # members 2 and 3 are replaced from 0 and 1
    parent = parent.tolist()
    assert parent[:2] == [0, 1] and set(parent[2:]) <= {0, 1}
    for m in range(K):
        assert torch.equal(nz.stats[m], stats[parent[m]]) and torch.equal(_bits(nz.scale[m]), _bits(scale[parent[m]])), m
        assert torch.equal(pop.flat[m, :pop.n_params], flat[parent[m], :pop.n_params]), m
    assert torch.equal(_bits(nz.ret_carry), _bits(ret_carry))          # the running returns belong to the envs
    s = pop.iterate()                                                   # and the population goes on
    assert all(np.isfinite(v).all() for v in s.values()), s
    assert (nz.stats[:, 0] == 3 * HORIZON * N_ENVS // K).all()
    env.close()


def _last_values(pop):
    """What PopulationPPO.collect() passes to the advantage estimation as the last values: the members on the kept observation."""
    last_v = torch.empty(N_ENVS, device=DEV)
    pop._act(pop.obs, None, None, None, last_v)
    return last_v


NORM_NAMES = ("stats", "scale", "ret_carry")


def _resume(make, names):
    env, a = make()
    for _ in range(2):
        a.iterate()
    sd = a.state_dict()
    for _ in range(2):
        a.iterate()
    torch.cuda.synchronize()
    want = {n: (getattr(a.rew_norm, n) if n in NORM_NAMES else getattr(a, n)).clone() for n in names}
    want_t = a.adam_t
    env.close()
    env2, b = make()
    b.iterate()                                                          # (another state: everything comes from the checkpoint)
    b.load_state_dict(sd)
    for _ in range(2):
        b.iterate()
    torch.cuda.synchronize()
    for n in names:
        got = getattr(b.rew_norm, n) if n in NORM_NAMES else getattr(b, n)
        assert torch.equal(_bits(got), _bits(want[n])), n
    assert b.adam_t == want_t
    return env2, b, sd


@pytest.mark.gpu
def test_ppo_resume_is_bit_for_bit():
    def make():
        env = _env(35)
        return env, PPO(env, horizon=HORIZON, seed=4, normalize_reward=True)

    env, agent, sd = _resume(make, ("flat", "adam_m", "adam_v", "obs", "rew_norm_b") + NORM_NAMES)
    assert sd["normalize_reward"] is True and sorted(sd["rew_norm"]) == ["clip", "eps", "members", "n_envs", "ret_carry", "scale", "stats"]
    env.close()
    env = _env(35)
    plain = PPO(env, horizon=HORIZON, seed=4)
    assert "normalize_reward" not in plain.state_dict() and "rew_norm" not in plain.state_dict()   # the keys of before
    assert sorted(set(sd) - set(plain.state_dict())) == ["normalize_reward", "rew_norm"]
    with pytest.raises(ValueError, match="normalize_reward"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="normalize_reward"):
        agent.load_state_dict(plain.state_dict())
    env.close()


@pytest.mark.gpu
def test_population_resume_is_bit_for_bit():
    def make():
        env = _env(36)
        return env, PopulationPPO(env, 4, horizon=HORIZON, seeds=[5, 6, 7, 8], gamma=[0.99, 0.9, 0.95, 0.8], normalize_reward=True)

    env, pop, sd = _resume(make, ("flat", "adam_m", "adam_v", "obs", "rew_norm_b") + NORM_NAMES)
    env.close()
    env = _env(36)
    plain = PopulationPPO(env, 4, horizon=HORIZON)
    assert "normalize_reward" not in plain.state_dict()
    with pytest.raises(ValueError, match="normalize_reward"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="normalize_reward"):
        pop.load_state_dict(plain.state_dict())
    env.close()
