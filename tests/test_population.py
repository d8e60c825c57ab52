"""Population PPO on the GPU (include/pcc_policy.h: pcc_policy_act_pop, pcc_ppo_minibatch_step_pop, pcc_gae_pop;
pcc_rl_amd.ppo.PopulationPPO): K learners on K slices of one env batch, one launch for all members where the single-policy entry
points take K.  Every comparison is torch.equal: the references are the existing entry points (pcc_policy_act,
pcc_ppo_minibatch_step, pcc_gae), called member by member.  Shapes are chosen to break slicing: member boundaries inside a
workgroup, a wavefront and a 32-sample tile (257 rows), one row, more tiles than the capped grid (70 000 samples)."""
import ctypes

import numpy as np
import pytest
import torch

import pcc_rl_amd
from pcc_rl_amd.native import lib
from pcc_rl_amd.ppo import MlpPolicy, PopulationPPO, gae_fused, population_permutations

K = 3
DEV = "cuda:0"
_ids = lambda s: "%d-%d-%d" % s
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _n_params(D, h1, h2):
    return 2 * (h1 * D + h1 + h2 * h1 + 2 * h2 + 1) + 1


def _stride(n_params):
    return (n_params + 63) // 64 * 64


PAD = 7.0   # what the padding of every [members][param_stride] block holds before a call -- and after it


def _param_block(shape, seed):
    """[K][stride] parameters of K different policies (log_std set off zero), padding = PAD; and the policies."""
    D, h1, h2 = shape
    n = _n_params(*shape)
    block = torch.full((K, _stride(n)), PAD, device=DEV)
    pols = []
    for m in range(K):
        torch.manual_seed(seed + m)
        pol = MlpPolicy(D, 1, (h1, h2))
        with torch.no_grad():
            pol.log_std.fill_(-0.3 - 0.2 * m)
        block[m, :n] = pol.flat_params().to(DEV)
        pols.append(pol.to(DEV))
    return block, n, pols


# ----------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.gpu
@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "mean"])
@pytest.mark.parametrize("n_m", [1, 257, 1000])
@pytest.mark.parametrize("shape", [(30, 32, 16), (30, 20, 10), (36, 64, 32), (120, 64, 64), (30, 48, 24)], ids=_ids)   # (the last: the generic kernel above 64 KB of dynamic LDS)
def test_forward_equals_member_calls(shape, n_m, with_noise):
    """The unrolled kernel, the older generic one and two tiled classes: all four outputs of one pcc_policy_act_pop equal three
    pcc_policy_act calls on the members' row slices; the padding of the parameter block is untouched."""
    D, h1, h2 = shape
    L = lib()
    block, n_par, _ = _param_block(shape, 10)
    before = block.clone()
    N = K * n_m
    g = torch.Generator().manual_seed(n_m)
    obs = torch.randn(N, D, generator=g).to(DEV)
    noise = torch.randn(N, generator=g).to(DEV) if with_noise else None
    got = [torch.full((N,), float("nan"), device=DEV) for _ in range(4)]
    rc = L.pcc_policy_act_pop(_p(obs), N, D, _p(block), block.stride(0), K, h1, h2, _p(noise), *[_p(t) for t in got], _stream())
    assert rc == 0
    want = [torch.full((N,), float("nan"), device=DEV) for _ in range(4)]
    for m in range(K):
        sl = slice(m * n_m, (m + 1) * n_m)
        params = block[m, :n_par].clone()                      # (a member's block alone, as a single-policy caller holds it)
        rc = L.pcc_policy_act(_p(obs[sl]), n_m, D, _p(params), h1, h2, _p(None if noise is None else noise[sl]),
                              *[_p(t[sl]) for t in want], _stream())
        assert rc == 0
    torch.cuda.synchronize()
    for name, a, b in zip(("mean", "act", "logp", "value"), got, want):
        assert torch.isfinite(b).all(), name
        assert torch.equal(a, b), (name, (a - b).abs().max().item())
    assert torch.equal(block, before)
    assert not torch.equal(got[0][:n_m], got[0][n_m:2 * n_m]) or n_m == 1   # (the members are different policies)
    # any subset of the outputs
    only_v = torch.full((N,), float("nan"), device=DEV)
    assert L.pcc_policy_act_pop(_p(obs), N, D, _p(block), block.stride(0), K, h1, h2, None, None, None, None, _p(only_v), _stream()) == 0
    assert torch.equal(only_v, want[3])


@pytest.mark.gpu
def test_forward_refuses_bad_arguments():
    D, h1, h2 = 30, 32, 16
    L = lib()
    block, n_par, _ = _param_block((D, h1, h2), 1)
    stride = block.stride(0)
    N = K * 8
    obs, out = torch.zeros(N, D, device=DEV), torch.zeros(N, device=DEV)
    call = lambda n, st, k, d=D: L.pcc_policy_act_pop(_p(obs), n, d, _p(block), st, k, h1, h2, None, None, _p(out), None, None, _stream())
    assert call(N, stride, K) == 0
    assert call(N, n_par - 1, K) == -1            # stride < n_params (3075)
    assert call(N, 3072, K) == -1                 # ... a multiple of 64 below it
    assert call(N, n_par, K) == -1                # not a multiple of 64
    assert call(N, stride + 32, K) == -1
    assert call(N, stride, 0) == -1               # n_members = 0
    assert call(N, stride, 1025) == -1
    assert call(N + 1, stride, K) == -1           # n_envs % n_members != 0
    assert call(N, stride, K, 129) == -2          # pcc_policy_act's code for an observation length outside the domain
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ update
HYPER = [[1e-3, 0.2, 0.01, 0.99, 0.95, 0, 0, 0], [0.0, 0.1, 0.0, 0.99, 0.95, 0, 0, 0], [3e-4, 0.3, 0.02, 0.99, 0.95, 0, 0, 0]]
# (samples per member, count, T, the three starts)
MINIBATCHES = [(5000, 3333, 8, (0, 800, 1667)), (70000, 70000, 7, (0, 0, 0)), (777, 1, 7, (0, 1, 776))]


@pytest.mark.gpu
@pytest.mark.parametrize("per_member,count,T,starts", MINIBATCHES, ids=lambda v: str(v) if isinstance(v, int) else None)
@pytest.mark.parametrize("shape", [(30, 32, 16), (36, 64, 32), (120, 64, 64), (7, 20, 10)], ids=_ids)
def test_update_equals_member_calls(shape, per_member, count, T, starts):
    """Three consecutive pcc_ppo_minibatch_step_pop calls against three pcc_ppo_minibatch_step calls each: parameters, Adam's
    moments, the gradient and the statistics, after every step; the lr = 0 member's parameters never move."""
    D, h1, h2 = shape
    L = lib()
    n_m = per_member // T
    assert n_m * T == per_member
    N, n = K * n_m, T * K * n_m
    block, n_par, pol_of = _param_block(shape, 20)
    stride = block.stride(0)
    start_params = block.clone()
    g = torch.Generator().manual_seed(per_member)
    obs = torch.randn(n, D, generator=g).to(DEV)
    act = (0.5 * torch.randn(n, generator=g)).to(DEV)
    adv = torch.randn(n, generator=g).to(DEV)
    ret = (2.0 * torch.randn(n, generator=g)).to(DEV)
    logp = torch.empty(n, device=DEV)
    perm = population_permutations(T, N, K, generator=g).to(DEV)
    with torch.no_grad():   # log-probabilities near each member's own policy: ratios around 1, some of them clipped
        for m in range(K):
            idx = perm[m]
            logp[idx] = pol_of[m].dist(obs[idx]).log_prob(act[idx].unsqueeze(1)).sum(-1) + 0.15 * torch.randn(per_member, generator=g).to(DEV)
    hyper = torch.tensor(HYPER, dtype=torch.float32, device=DEV)
    sf = L.pcc_ppo_scratch_floats(D, h1, h2)
    scratch = torch.empty(K * sf, device=DEV)
    full = lambda: torch.full((K, stride), PAD, device=DEV)
    pm, pv, pg = full(), full(), full()
    pm[:, :n_par] = 0.0
    pv[:, :n_par] = 0.0
    pstats = torch.full((K, 4), float("nan"), device=DEV)
    # the references: every member's own contiguous block, moments, scratch
    rp = [block[m, :n_par].clone() for m in range(K)]
    rm, rv = [torch.zeros(n_par, device=DEV) for _ in range(K)], [torch.zeros(n_par, device=DEV) for _ in range(K)]
    rg, rs = [torch.zeros(n_par, device=DEV) for _ in range(K)], [torch.zeros(4, device=DEV) for _ in range(K)]
    rscratch = torch.empty(sf, device=DEV)
    for step, start in enumerate(starts, 1):
        scratch.fill_(float("nan"))
        rc = L.pcc_ppo_minibatch_step_pop(_p(obs), _p(act), _p(logp), _p(adv), _p(ret), _p(perm), perm.stride(0), start, count, D, h1, h2,
                                          _p(block), _p(pm), _p(pv), stride, K, _p(hyper), step, 0.9, 0.999, 1e-5, _p(scratch), _p(pg),
                                          _p(pstats), _stream())
        assert rc == 0
        for m in range(K):
            rscratch.fill_(float("nan"))
            lr, clip, ent = HYPER[m][:3]
            rc = L.pcc_ppo_minibatch_step(_p(obs), _p(act), _p(logp), _p(adv), _p(ret), _p(perm[m]), start, count, D, h1, h2, _p(rp[m]),
                                          _p(rm[m]), _p(rv[m]), step, lr, 0.9, 0.999, 1e-5, clip, ent, _p(rscratch), _p(rg[m]), _p(rs[m]),
                                          _stream())
            assert rc == 0
        torch.cuda.synchronize()
        for m in range(K):
            for name, a, b in (("params", block, rp), ("adam_m", pm, rm), ("adam_v", pv, rv), ("grad", pg, rg)):
                assert torch.isfinite(b[m]).all(), (name, m, step)
                assert torch.equal(a[m, :n_par], b[m]), (name, m, step, (a[m, :n_par] - b[m]).abs().max().item())
                assert (a[m, n_par:] == PAD).all(), (name, m, step)
            assert torch.equal(pstats[m], rs[m]), (m, step, pstats[m], rs[m])
            assert rg[m].abs().max() > 0
        assert torch.equal(block[1], start_params[1])                       # lr = 0: gradient only
        assert not torch.equal(block[0], start_params[0]) and not torch.equal(block[2], start_params[2])
    if count >= 64:
        assert 0.0 < float(pstats[:, 2].min()) and float(pstats[:, 2].max()) < 1.0   # some ratios clipped, not all


@pytest.mark.gpu
def test_update_refuses_bad_arguments():
    D, h1, h2 = 30, 32, 16
    L = lib()
    block, n_par, _ = _param_block((D, h1, h2), 1)
    stride, n = block.stride(0), K * 64
    z = torch.zeros(n, device=DEV)
    obs = torch.zeros(n, D, device=DEV)
    perm = population_permutations(1, n, K).to(DEV)
    hyper = torch.tensor(HYPER, dtype=torch.float32, device=DEV)
    m, v = torch.zeros_like(block), torch.zeros_like(block)
    scratch = torch.empty(K * L.pcc_ppo_scratch_floats(D, h1, h2), device=DEV)

    def call(perm_=perm, st=stride, k=K, step=1, m_=m, count=64):
        return L.pcc_ppo_minibatch_step_pop(_p(obs), _p(z), _p(z), _p(z), _p(z), _p(perm_), 64, 0, count, D, h1, h2, _p(block), _p(m_), _p(v),
                                            st, k, _p(hyper), step, 0.9, 0.999, 1e-5, _p(scratch), None, None, _stream())
    assert call() == 0
    assert call(perm_=None) == -1                 # perm is required
    assert call(st=n_par) == -1 and call(st=3072) == -1
    assert call(k=0) == -1
    assert call(step=0) == -1                     # adam_step >= 1 always
    assert call(m_=None) == -1
    assert call(count=0) == -1
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------------- GAE
@pytest.mark.gpu
def test_gae_equals_member_calls():
    T, n_m = 7, 257
    N = K * n_m
    g = torch.Generator().manual_seed(9)
    rew, val, last = torch.randn(T, N, generator=g).to(DEV), torch.randn(T, N, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    done = (torch.rand(T, N, generator=g) < 0.15).to(DEV)
    hyper = torch.tensor([[0, 0, 0, 0.99, 0.95, 0, 0, 0], [0, 0, 0, 0.9, 1.0, 0, 0, 0], [0, 0, 0, 0.999, 0.5, 0, 0, 0]], dtype=torch.float32,
                         device=DEV)
    adv, ret = torch.full((T, N), float("nan"), device=DEV), torch.full((T, N), float("nan"), device=DEV)
    rc = lib().pcc_gae_pop(_p(rew), _p(val), _p(done.view(torch.uint8)), _p(last), T, N, K, _p(hyper), _p(adv), _p(ret), _stream())
    assert rc == 0
    for m in range(K):
        c = slice(m * n_m, (m + 1) * n_m)
        a, r = gae_fused(rew[:, c].contiguous(), val[:, c].contiguous(), done[:, c].contiguous(), last[c].contiguous(),
                         float(hyper[m, 3]), float(hyper[m, 4]))
        assert torch.equal(adv[:, c], a) and torch.equal(ret[:, c], r), m
    assert torch.isfinite(adv).all() and not torch.equal(adv[:, :n_m], adv[:, n_m:2 * n_m])
    assert lib().pcc_gae_pop(_p(rew), _p(val), _p(done.view(torch.uint8)), _p(last), T, N, 2, _p(hyper), _p(adv), _p(ret), _stream()) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- PopulationPPO end to end
POOLS = (2, 8, 32)   # (fixed ring pools: the library's default depends on the free device memory, and a snapshot needs equal pools)


def _env(n, seed, **kw):
    return pcc_rl_amd.BatchedNetworkEnv(n, device=DEV, seed=seed, ring_pools=POOLS, **kw)


@pytest.mark.gpu
def test_rollout_slices_equal_single_policy_loops():
    """collect() of 3 members x 512 envs over 12 steps: every member's rows equal a loop of the existing public pieces
    (act_fused, step_into, gae_fused) on a handle of its own 512 envs (env_gid_base = m * 512) with the member's policy."""
    n_m, T = 512, 12
    N = K * n_m
    gammas, lams = [0.99, 0.9, 0.97], [0.95, 0.8, 1.0]
    env = _env(N, 5)
    pop = PopulationPPO(env, K, horizon=T, gamma=gammas, lam=lams, seeds=[4, 5, 6])
    noise = torch.randn((T, N), device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    start = [{k: v.detach().clone() for k, v in p.state_dict().items()} for p in pop.policies]
    obs_b, act_b, logp_b, adv, ret, rew_b = pop.collect(noise=noise)
    torch.cuda.synchronize()
    env.close()
    D = obs_b.shape[2]
    for m in range(K):
        c = slice(m * n_m, (m + 1) * n_m)
        e = _env(n_m, 5, env_gid_base=m * n_m)
        pol = MlpPolicy(D, 1, (32, 16)).to(DEV)
        pol.load_state_dict(start[m])
        params = pol.flat_params()
        assert torch.equal(params, pop.flat[m, :pop.n_params])
        o = torch.empty((T + 1, n_m, D), device=DEV)
        a, lp, v, r = (torch.empty((T, n_m), device=DEV) for _ in range(4))
        d = torch.empty((T, n_m), dtype=torch.bool, device=DEV)
        o[0] = e.reset()
        for t in range(T):
            pol.act_fused(o[t], True, params, noise[t, c].contiguous(), (a[t], lp[t], v[t]))
            e.step_into(a[t].reshape(n_m, 1), o[t + 1], r[t], d[t])
        _, _, last_v = pol.act_fused(o[T], stochastic=False, params=params)
        e.check_flags()
        ad, rt = gae_fused(r, v, d, last_v, gammas[m], lams[m])
        torch.cuda.synchronize()
        e.close()
        for name, x, y in (("obs", obs_b[:, c], o[:T]), ("act", act_b[:, c, 0], a), ("logp", logp_b[:, c], lp), ("value", pop.val_b[:, c], v),
                           ("reward", rew_b[:, c], r), ("done", pop.done_b[:, c], d), ("adv", adv[:, c], ad), ("ret", ret[:, c], rt),
                           ("next obs", pop.obs[c], o[T])):
            assert torch.equal(x, y), (name, m)
        assert torch.isfinite(ad).all()


def _run(lr, seeds, iters, horizon=32, load=None):
    env = _env(K * 512, 12)
    pop = PopulationPPO(env, K, horizon=horizon, lr=lr, seeds=seeds)
    start = pop.flat.clone()
    if load is not None:
        pop.load_state_dict(load)
    returns = []
    for it in range(iters):
        returns.append(pop.iterate()["mean_step_reward"])
    torch.cuda.synchronize()
    return env, pop, start, returns


@pytest.mark.gpu
def test_members_are_isolated():
    """Two runs that differ in member 1's learning rate and seed only: members 0 and 2 end with the same bits; the member with
    lr = 0 ends where it started.  (The LAST member's seed is the same in both runs on purpose: the constructor seeds torch's
    generators member by member, as PPO(seed=...) does, and leaves them seeded by seeds[-1]; the rollout's noise and the
    permutations are drawn from there, so both runs draw the same ones.)"""
    ea, a, start_a, ra = _run([1e-3, 1e-3, 0.0], [0, 1, 2], 2)
    eb, b, start_b, rb = _run([1e-3, 3e-4, 0.0], [0, 7, 2], 2)
    assert a.adam_t == b.adam_t and a.adam_t >= 2 * a.epochs
    assert torch.equal(a.flat[0], b.flat[0]) and torch.equal(a.flat[2], b.flat[2])
    assert not torch.equal(a.flat[1], b.flat[1])
    assert torch.equal(a.flat[2], start_a[2])                                # lr = 0
    assert not torch.equal(a.flat[0], start_a[0])
    assert [r[0] for r in ra] == [r[0] for r in rb] and [r[2] for r in ra] == [r[2] for r in rb]
    assert torch.equal(a.policies[0].pi[0].weight, b.policies[0].pi[0].weight)   # (the modules are views of the rows)
    ea.close(); eb.close()


@pytest.mark.gpu
def test_resume_is_bit_for_bit():
    lr, seeds = [1e-3, 3e-4, 1e-3], [3, 4, 5]
    env, pop, _, _ = _run(lr, seeds, 2)
    sd = pop.state_dict()
    want = [pop.iterate()["mean_step_reward"] for _ in range(2)]
    want_flat, want_m, want_t = pop.flat.clone(), pop.adam_m.clone(), pop.adam_t
    env.close()
    env2, other, _, got = _run(lr, [9, 9, 9], 2, load=sd)                    # (another start: everything comes from the state)
    assert got == want
    assert torch.equal(other.flat, want_flat) and torch.equal(other.adam_m, want_m) and other.adam_t == want_t
    env2.close()


@pytest.mark.gpu
def test_a_population_learns():
    """4 members x 1 024 envs, horizon 400, 10 iterations, default hyper-parameters, seeds 0..3: the bound tests/test_ppo.py
    applies to one seed at this size (the last three iterations > 1.5 x the first two), on the mean over the members."""
    env = pcc_rl_amd.BatchedNetworkEnv(4096, device=DEV, seed=3)
    pop = PopulationPPO(env, 4, horizon=400, seeds=[0, 1, 2, 3])
    returns = np.array([pop.iterate()["mean_step_reward"] for _ in range(10)]) * env.max_steps   # [iteration][member]
    env.check_flags()
    print("returns per iteration and member:\n%s" % np.round(returns, 1))
    assert np.isfinite(returns).all()
    first, last = returns[:2].mean(), returns[-3:].mean()
    print("mean over members: first two %.1f, last three %.1f" % (first, last))
    assert last > 1.5 * first, returns
    env.close()
