"""Keyed random streams of the learners on the GPU (include/pcc_policy.h: pcc_rollout_noise_pop, pcc_sample_order_pop,
pcc_adv_standardise_pop and their stand-alone forms; pcc_rl_amd.streams.LearnerStreams; PPO / PopulationPPO(rng="philox"); DESIGN.md
section 25).  The kernels are held to the numpy restatement of tests/models/learner_streams_model.py -- the order and the Philox
words exactly, the standardisation bit for bit, the normals within one float32 spacing of the float64 model -- on the smallest shapes
that can go wrong: member sizes 1, 5 and 257 (a member boundary inside a wavefront and inside a 4-env Philox block), 260 (the float4
stores), one row, every even-bit domain the sizes reach.  Then the point of the option: a member of a population, the same seed as a
population of one and as a PPO on a handle of the member's env ids compute the same bits, whatever torch's generators did meanwhile,
across a checkpoint and an evolve()."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import learner_streams_model as model   # noqa: E402

import pcc_rl_amd   # noqa: E402
from pcc_rl_amd.native import lib   # noqa: E402
from pcc_rl_amd.ppo import PPO, PopulationPPO   # noqa: E402
from pcc_rl_amd.streams import LearnerStreams, key_from_seed   # noqa: E402

DEV = "cuda:0"
SEEDS = [4, 5, 6]
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


# ------------------------------------------------------------------------------------------------------------ sample order
@pytest.mark.gpu
@pytest.mark.parametrize("n_m", [1, 5, 257])
@pytest.mark.parametrize("K", [1, 3])
def test_sample_order_equals_the_model(K, n_m):
    """T in {1, 7, 12}: n = 1, 5, 7, 12, 35, 60, 257, 1799, 3084 -- the domains 4^0 .. 4^6.  Every row is the model's, a permutation of
    the member's own columns; a perm_stride above n leaves the padding untouched; the stand-alone call gives the member's local order."""
    st = LearnerStreams(SEEDS[:K], K * n_m, DEV)
    N = K * n_m
    for T in (1, 7, 12):
        n = T * n_m
        for it, ep in ((1, 0), (2, 3)):
            want = model.order_global(st.host_keys, it, ep, T, N)
            got = st.order(T, it, ep)
            assert got.shape == (K, n) and torch.equal(got.cpu(), torch.from_numpy(want)), (T, it, ep)
        g = got.cpu().numpy()
        for m in range(K):
            assert sorted(g[m].tolist()) == sorted((t * N + m * n_m + e) for t in range(T) for e in range(n_m))
        padded = torch.full((K, n + 3), -7, dtype=torch.int64, device=DEV)
        st.order(T, 2, 3, out=padded)
        assert torch.equal(padded[:, :n], got) and (padded[:, n:] == -7).all()
        alone = torch.full((n,), -7, dtype=torch.int64, device=DEV)
        m = K - 1
        assert lib().pcc_sample_order(_p(alone), T, n_m, st.host_keys[m], 2, 3, _stream()) == 0
        assert torch.equal(alone.cpu(), torch.from_numpy(model.order_local(st.host_keys[m], 2, 3, n)))   # (one member: global = local)
        t_, e_ = alone // n_m, alone % n_m
        assert torch.equal(t_ * N + m * n_m + e_, got[m])


# ------------------------------------------------------------------------------------------------------------------- noise
@pytest.mark.gpu
@pytest.mark.parametrize("n_m", [1, 5, 257, 260])
@pytest.mark.parametrize("K", [1, 3])
def test_noise_equals_the_model(K, n_m):
    """The raw Philox words are the model's exactly; the normals are within one float32 spacing of the float64 model (the device's
    float64 log, sqrt and sincospi are a few ulp64: only the final rounding can differ); a member's values are the stand-alone call's
    with its key.  n_m = 257: a member boundary inside a wavefront and a 4-env block; 260: the float4 stores; T = 1 and 7."""
    st = LearnerStreams(SEEDS[:K], K * n_m, DEV)
    N = K * n_m
    exact = total = 0
    for T, it in ((1, 1), (7, 3)):
        words = torch.full((T, N), -1, dtype=torch.int32, device=DEV)
        z = st.noise(T, it, words=words)
        plain = st.noise(T, it)
        assert torch.equal(z, plain)                                   # the debug output changes nothing
        got, w = z.cpu().numpy(), words.cpu().numpy().view(np.uint32)
        for m in range(K):
            c = slice(m * n_m, (m + 1) * n_m)
            assert np.array_equal(w[:, c], model.noise_words(st.host_keys[m], it, T, n_m)), (m, T)
            want = model.noise64(st.host_keys[m], it, T, n_m)
            want32 = want.astype(np.float32)
            assert (np.abs(got[:, c].astype(np.float64) - want) <= np.spacing(np.abs(want32))).all(), (m, T)
            exact += int((got[:, c] == want32).sum())
            total += want32.size
            alone = torch.empty((T, n_m), device=DEV)
            assert lib().pcc_rollout_noise(_p(alone), None, T, n_m, st.host_keys[m], it, _stream()) == 0
            assert torch.equal(alone, z[:, c])
        if K == 3 and n_m > 1:
            assert not np.array_equal(got[:, :n_m], got[:, n_m:2 * n_m])   # (the members' streams differ)
    print("exact float32 matches: %d of %d" % (exact, total))
    other = st.noise(7, 4)
    assert not torch.equal(other, z)                                   # another iteration: other draws


# --------------------------------------------------------------------------------------------------------- standardisation
@pytest.mark.gpu
@pytest.mark.parametrize("T,K,n_m", [(7, 3, 257), (12, 3, 5), (1, 1, 1000), (3, 2, 70000), (9, 3, 1)])
def test_standardise_equals_the_model(T, K, n_m):
    """torch.equal with the model's float32 output, the moments bit-equal in float64, a member bit-equal to the stand-alone call on a
    contiguous copy of its columns, and in place.  (3, 2, 70000): more than 256 workgroups per member, so the merge's sub-lanes add
    more than one partial each."""
    g = torch.Generator().manual_seed(T * 1000 + n_m)
    scale = torch.tensor([1.0, 10.0, 0.1])[:K].repeat_interleave(n_m)
    adv = (torch.randn(T, K * n_m, generator=g) * scale + 3.0).to(DEV)
    st = LearnerStreams(SEEDS[:K], K * n_m, DEV)
    before = adv.clone()
    out = st.standardise(adv)
    want, moments = model.standardise(adv.cpu().numpy(), K)
    assert torch.equal(adv, before)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    assert np.array_equal(st.moments.cpu().numpy().view(np.int64), moments.view(np.int64))
    L = lib()
    for m in range(K):
        a = adv[:, m * n_m:(m + 1) * n_m].contiguous()
        scratch = torch.empty(L.pcc_adv_standardise_scratch_doubles(T, n_m, 1), dtype=torch.float64, device=DEV)
        mom, o = torch.zeros(2, dtype=torch.float64, device=DEV), torch.empty_like(a)
        assert L.pcc_adv_standardise(_p(a), T, n_m, _p(scratch), _p(mom), _p(o), _stream()) == 0
        assert torch.equal(o, out[:, m * n_m:(m + 1) * n_m]) and torch.equal(mom, st.moments[m])
    mom = st.moments.clone()
    st.standardise(adv, out=adv)                                       # out == adv
    assert torch.equal(adv, out) and torch.equal(st.moments, mom)


@pytest.mark.gpu
def test_standardise_edges():
    st = LearnerStreams(SEEDS, 12, DEV)
    out = st.standardise(torch.full((5, 12), 2.5, device=DEV))        # constant advantages: all 0
    assert (out == 0.0).all() and (st.moments[:, 0] == 2.5).all() and (st.moments[:, 1] == 0.0).all()
    st = LearnerStreams(SEEDS, 3, DEV)
    out = st.standardise(torch.tensor([[1.0, 2.0, 3.0]], device=DEV))  # one sample per member: NaN, as torch's formula gives
    assert torch.isnan(out).all() and torch.isnan(st.moments[:, 1]).all() and st.moments[:, 0].tolist() == [1.0, 2.0, 3.0]


# ---------------------------------------------------------------------------------------------------------------- trainers
POOLS = (2, 8, 32)   # (fixed ring pools: the library's default depends on the free device memory, and a snapshot needs equal pools)
N_M, T_ROLL = 512, 12


def _env(n, **kw):
    return pcc_rl_amd.BatchedNetworkEnv(n, device=DEV, seed=5, ring_pools=POOLS, **kw)


def _keep(agent, rows):
    """What a run is compared by: per member the parameters, Adam's moments and the rollout's rows of the last iteration."""
    K = getattr(agent, "members", 1)
    n_par = agent.n_params if isinstance(agent, PopulationPPO) else agent.flat.numel()
    flat, am, av = (x.reshape(K, -1)[:, :n_par].clone() for x in (agent.flat, agent.adam_m, agent.adam_v))
    obs, act, logp, adv, ret, rew = rows
    out = []
    for m in range(K):
        c = slice(m * N_M, (m + 1) * N_M)
        out.append({"flat": flat[m], "adam_m": am[m], "adam_v": av[m], "obs": obs[:, c].clone(), "act": act[:, c].clone(),
                    "logp": logp[:, c].clone(), "adv": adv[:, c].clone(), "ret": ret[:, c].clone(), "rew": rew[:, c].clone(),
                    "val": agent.val_b[:, c].clone(), "done": agent.done_b[:, c].clone(), "next_obs": agent.obs[c].clone()})
    return out


def _iterate(agent, iters, between=None):
    rows = None
    for i in range(iters):
        rows = agent.collect()
        agent.update(*rows[:5])
        if between is not None:
            between(i)
    torch.cuda.synchronize()
    return rows


def _run_population(seeds, iters=2, between=None, **kw):
    env = _env(len(seeds) * N_M)
    pop = PopulationPPO(env, len(seeds), horizon=T_ROLL, seeds=seeds, rng="philox", **kw)
    got = _keep(pop, _iterate(pop, iters, between))
    env.close()
    return got


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.fixture(scope="module")
def population_run():
    """3 members x 512 envs x 12 steps, two iterations, seeds 4, 5, 6: computed once, left unchanged."""
    return _run_population(SEEDS)


@pytest.mark.gpu
def test_a_member_equals_a_population_of_one_and_a_ppo(population_run):
    """Member m's parameters, Adam moments and rollout rows after two iterations equal PopulationPPO(members=1, seeds=[s_m]) and
    PPO(seed=s_m) on a handle with env_gid_base = m * 512."""
    for m, seed in enumerate(SEEDS):
        env = _env(N_M, env_gid_base=m * N_M)
        one = PopulationPPO(env, 1, horizon=T_ROLL, seeds=[seed], rng="philox")
        got = _keep(one, _iterate(one, 2))[0]
        env.close()
        _same(population_run[m], got, "population of one, member %d" % m)
        env = _env(N_M, env_gid_base=m * N_M)
        ppo = PPO(env, horizon=T_ROLL, seed=seed, rng="philox")
        got = _keep(ppo, _iterate(ppo, 2))[0]
        assert ppo.iteration == 2 and ppo.adam_t == one.adam_t
        env.close()
        _same(population_run[m], got, "PPO, member %d" % m)
    assert not torch.equal(population_run[0]["flat"], population_run[1]["flat"])
    assert torch.isfinite(population_run[0]["flat"]).all() and torch.isfinite(population_run[2]["adv"]).all()


@pytest.mark.gpu
def test_members_in_another_order_and_beside_torch_draws(population_run):
    """The same learners in other slots -- the envs stay with the slots, so a learner is compared on the same env ids: seeds (9, 5, 4)
    keeps member 1 where it was beside other neighbours -- and with extra draws from torch's generators between the iterations."""
    def between(i):
        torch.randn(1000, device=DEV)
        torch.rand(7)
        torch.manual_seed(100 + i)
    got = _run_population([9, 5, 4], between=between)
    _same(population_run[1], got[1], "member 1 beside other neighbours")
    assert not torch.equal(population_run[0]["flat"], got[0]["flat"])
    # a population of two sizes: member 0 of (4, 5) is member 0 of (4, 5, 6)
    got = _run_population(SEEDS[:2], between=between)
    _same(population_run[0], got[0], "member 0 of a population of two")
    _same(population_run[1], got[1], "member 1 of a population of two")


@pytest.mark.gpu
def test_given_noise_and_orders_take_precedence():
    env = _env(3 * N_M)
    pop = PopulationPPO(env, 3, horizon=T_ROLL, seeds=SEEDS, rng="philox")
    noise = torch.zeros((T_ROLL, 3 * N_M), device=DEV)
    rows = pop.collect(noise=noise)
    torch.cuda.synchronize()
    assert pop.iteration == 1
    mean_act = rows[1].clone()
    n = T_ROLL * N_M
    perms = [pop.streams.order(T_ROLL, 77, e) for e in range(pop.epochs)]
    pop.update(*rows[:5], perms=perms)
    a = pop.flat.clone()
    env.close()
    env = _env(3 * N_M)
    pop = PopulationPPO(env, 3, horizon=T_ROLL, seeds=SEEDS, rng="philox")
    rows = pop.collect(noise=noise)
    assert torch.equal(rows[1], mean_act)
    pop.update(*rows[:5])                       # the iteration's own orders: other minibatches
    torch.cuda.synchronize()
    assert not torch.equal(pop.flat, a) and perms[0].shape == (3, n)
    env.close()


@pytest.mark.gpu
def test_resume_is_bit_for_bit(population_run):
    """Checkpoint after iteration 1, evolve() on both sides, continue in a fresh object built from other seeds: the same bits; the keys
    stay with their slots through evolve().  And PPO across a checkpoint."""
    scores = [1.0, 3.0, 2.0, 0.0]
    env = _env(4 * N_M)
    pop = PopulationPPO(env, 4, horizon=T_ROLL, seeds=SEEDS + [7], rng="philox")
    _iterate(pop, 1)
    sd = pop.state_dict()
    assert sd["rng"] == "philox" and sd["iteration"] == 1 and sd["streams"]["keys"] == [key_from_seed(s) for s in SEEDS + [7]]
    keys = pop.streams.keys.clone()
    parent, _ = pop.evolve(scores, frac=0.25)
    assert parent.tolist() == [0, 1, 2, 1] and torch.equal(pop.streams.keys, keys)
    want = _keep(pop, _iterate(pop, 1))
    env.close()
    env = _env(4 * N_M)
    other = PopulationPPO(env, 4, horizon=T_ROLL, seeds=[9, 9, 9, 9], rng="philox")
    other.load_state_dict(sd)
    other.evolve(scores, frac=0.25)
    got = _keep(other, _iterate(other, 1))
    assert other.iteration == 2
    for m in range(4):
        _same(want[m], got[m], "resumed member %d" % m)
    assert not torch.equal(want[3]["act"], want[1]["act"])     # the replaced member has its parent's weights and its own stream
    env.close()
    # PPO: iteration 1, checkpoint, iteration 2 == the fixture's member 0 (seed 4 on env ids 0 ..)
    env = _env(N_M)
    ppo = PPO(env, horizon=T_ROLL, seed=SEEDS[0], rng="philox")
    _iterate(ppo, 1)
    sd = ppo.state_dict()
    env.close()
    env = _env(N_M)
    fresh = PPO(env, horizon=T_ROLL, seed=123, rng="philox")
    fresh.load_state_dict(sd)
    got = _keep(fresh, _iterate(fresh, 1))[0]
    _same(population_run[0], got, "PPO resumed")
    torch_mode = PPO(env, horizon=T_ROLL, seed=123)
    with pytest.raises(ValueError, match="written with rng="):
        torch_mode.load_state_dict(sd)
    with pytest.raises(ValueError, match="written with rng="):
        fresh.load_state_dict(torch_mode.state_dict())
    env.close()


@pytest.mark.gpu
def test_every_rollout_path_and_option():
    """rng="philox" with the policy inside the env's launches and over a GroupedNetworkEnv gives the fused loop's bits (the noise is
    the same tensor whichever path reads it), and runs with every other option switched on."""
    ref = None
    for kind in ("loop", "in_step", "grouped"):
        env = (pcc_rl_amd.GroupedNetworkEnv(2 * N_M, 2, device=DEV, seed=5, ring_pools=POOLS) if kind == "grouped" else _env(2 * N_M))
        ppo = PPO(env, horizon=T_ROLL, seed=3, rng="philox", policy_in_step=kind == "in_step")
        _iterate(ppo, 2)
        got = (ppo.flat.clone(), ppo.adam_m.clone(), ppo.val_b.clone())
        env.close()
        if ref is None:
            ref = got
        for a, b in zip(ref, got):
            assert torch.equal(a, b), kind
    opts = dict(normalize_obs=True, normalize_reward=True, track_episodes=True, target_kl=0.05, max_grad_norm=0.5)
    env = _env(3 * N_M)
    pop = PopulationPPO(env, 3, horizon=T_ROLL, seeds=SEEDS, rng="philox", **opts)
    stats = [pop.iterate() for _ in range(2)]
    assert torch.isfinite(pop.flat).all() and np.isfinite(stats[-1]["mean_step_reward"]).all() and pop.iteration == 2
    env.close()
    env = _env(N_M)
    ppo = PPO(env, horizon=T_ROLL, seed=SEEDS[0], rng="philox", **opts)
    one = [ppo.iterate() for _ in range(2)]
    # ... and there too the single policy is the population's member 0
    assert torch.equal(ppo.flat, pop.flat[0, :pop.n_params]) and one[-1]["approx_kl"] == stats[-1]["approx_kl"][0]
    env.close()


@pytest.mark.gpu
def test_the_default_draws_from_torch():
    """rng="torch" (the default) still takes its noise from torch's generator: reseeding it repeats a rollout, and the streams are not
    made."""
    env = _env(N_M)
    ppo = PPO(env, horizon=4, seed=1)
    assert ppo.rng == "torch" and ppo.streams is None and "rng" not in ppo.state_dict()
    sd = ppo.state_dict()
    a = ppo.collect()[1].clone()
    ppo.load_state_dict(sd)
    torch.manual_seed(99)
    b = ppo.collect()[1].clone()
    ppo.load_state_dict(sd)
    c = ppo.collect()[1].clone()
    assert torch.equal(a, c) and not torch.equal(a, b) and ppo.iteration == 0
    env.close()
