"""The fused PPO update and policy forward for any --arch and observation length of the library's domain
(include/pcc_policy.h: pcc_ppo_supported -- up to 128 observations, two hidden layers up to 64 wide): the tiled kernels of
pcc-rl_amd/csrc/pcc_mlp_tiles.h next to the fixed-shape ones.

CPU: the domain, the scratch size, and the compiler's resource report (no scratch memory, no spilled vector register in any
instantiation of the new kernels).  GPU: gradient, statistics, determinism, optimiser steps, forward, PPO end to end and
closed-loop rollouts for shapes that had no kernel before -- with the bounds of tests/test_ppo.py and tests/test_rollout.py.
No shape is skipped: one the library does not support fails."""
import ctypes
import warnings

import pytest
import torch

import pcc_rl_amd
from pcc_rl_amd import native
from pcc_rl_amd.native import lib
from pcc_rl_amd.ppo import PPO, MlpPolicy, ppo_loss

# (obs_dim, h1, h2)
SHAPES = [(36, 32, 16), (60, 32, 16), (36, 64, 32), (120, 64, 64), (128, 64, 64), (7, 20, 10), (45, 48, 24), (1, 1, 1)]
MINIBATCHES = [(5000, 3333), (70000, 70000), (777, 1), (1000, 64), (4097, 4097)]
_ids = lambda s: "%d-%d-%d" % s


def _n_net(D, h1, h2):
    return h1 * D + h1 + h2 * h1 + h2 + h2 + 1


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_supported_domain():
    L = lib()
    for s in [(30, 32, 16), (36, 32, 16), (60, 64, 32), (120, 64, 64), (128, 64, 64), (1, 1, 1), (7, 20, 10), (45, 48, 24)]:
        assert L.pcc_ppo_supported(*s) == 1, s
        assert L.pcc_ppo_scratch_floats(*s) >= 2 * _n_net(*s) + 5 > 0, s
    for s in [(0, 32, 16), (129, 32, 16), (30, 0, 16), (30, 32, 0), (30, 65, 16), (30, 32, 65)]:
        assert L.pcc_ppo_supported(*s) == 0, s


def test_every_test_shape_is_supported():
    for s in SHAPES + [(33, 32, 16)]:
        assert lib().pcc_ppo_supported(*s) == 1, s


def test_tiled_kernels_use_no_scratch(tmp_path):
    """A build into a temporary file: every instantiation of the tiled gradient and forward kernels is in the compiler's
    resource report with 0 bytes of scratch and 0 spilled vector registers; the fixed-shape kernels are still there."""
    import json
    from pcc_rl_amd import build as pbuild
    out = str(tmp_path / "libpcc_sim_res.so")
    pbuild.build_library(force=True, out=out)
    res = json.load(open(out + ".resources.json"))
    for kern in ("ppo_grad_tiled_kernel", "policy_act_tiled_kernel"):
        for D in (32, 64, 128):
            for h in ((32, 32), (64, 32), (64, 64)):
                name = "pcc_tiles::%s<%d, %d, %d>" % (kern, D, h[0], h[1])
                assert name in res, name
                assert res[name]["scratch"] == 0 and res[name]["vgpr_spills"] == 0, (name, res[name])
                assert res[name]["lds"] <= 160 * 1024
    for name in ("ppo_grad_mfma_kernel<30, 32, 16>", "policy_act_fixed_kernel<30, 32, 16>"):
        assert res[name]["scratch"] == 0 and res[name]["vgpr_spills"] == 0, (name, res[name])
    # the unchanged kernels' figures (the same as at the parent commit)
    assert (res["ppo_grad_mfma_kernel<30, 32, 16>"]["vgprs"], res["ppo_grad_mfma_kernel<30, 32, 16>"]["lds"]) == (256, 52736)
    assert res["policy_act_fixed_kernel<30, 32, 16>"]["vgprs"] == 87


# ----------------------------------------------------------------------------------------------------------------- GPU
def _rollout_like(n, D, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    obs = torch.randn(n, D, generator=g).to(dev)
    act = (0.5 * torch.randn(n, 1, generator=g)).to(dev)
    logp = (-1.0 + 0.3 * torch.randn(n, generator=g)).to(dev)
    adv = torch.randn(n, generator=g).to(dev)
    adv[::97] = 0.0
    ret = (2.0 * torch.randn(n, generator=g)).to(dev)
    return obs, act, logp, adv, ret


class _Env(object):   # what PPO.__init__ needs of an env, without a simulator behind it
    def __init__(self, D, dev):
        self.obs_dim, self.device, self.n_senders, self.n_envs = D, dev, 1, 8

    def reset(self):
        return torch.zeros(self.n_envs, self.obs_dim, device=self.device)


def _agent(shape, dev, seed=5):
    D, h1, h2 = shape
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        agent = PPO(_Env(D, dev), arch=(h1, h2), seed=seed)
    assert agent.fused_update, shape
    return agent


def _minibatch(agent, shape, n, dev, spread=0.15):
    obs, act, logp, adv, ret = _rollout_like(n, shape[0], dev, 11)
    with torch.no_grad():                                     # log-probabilities near the policy's own: ratios around 1,
        logp = agent.policy.dist(obs).log_prob(act).sum(-1) + spread * torch.randn(n, device=dev)   # some of them clipped
    return obs, act, logp, adv, ret


def _flat_grads(pol):
    def net(seq):
        return [p.grad.reshape(-1) for m in seq if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]
    return torch.cat(net(pol.pi) + [pol.log_std.grad.reshape(-1)] + net(pol.vf))


@pytest.mark.gpu
@pytest.mark.parametrize("with_perm", [True, False], ids=["perm", "noperm"])
@pytest.mark.parametrize("n,count", MINIBATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gradient_matches_float64_autograd(shape, n, count, with_perm):
    """pcc_ppo_minibatch_step's gradient (lr = 0) against float64 autograd of ppo_loss on the same minibatch: the bound of
    tests/test_ppo.py, max|g - want| <= 1e-5 max|want| + 1e-7, and its statistics bounds."""
    dev = torch.device("cuda:0")
    D, h1, h2 = shape
    agent = _agent(shape, dev)
    with torch.no_grad():
        agent.policy.log_std.fill_(-0.4)
    obs, act, logp, adv, ret = _minibatch(agent, shape, n, dev)
    perm = torch.randperm(n, device=dev) if with_perm else None
    g = torch.zeros_like(agent.flat)
    start = min(5, n - count)
    agent.minibatch_step_fused(obs, act.reshape(n), logp, adv, ret, perm, start, count, lr=0.0, grad_out=g)
    stats = agent.stats_buf.tolist()
    idx = perm[start:start + count] if with_perm else torch.arange(start, start + count, device=dev)
    pol64 = MlpPolicy(D, 1, (h1, h2)).to(dev).double()
    pol64.load_state_dict({k: v.double() for k, v in agent.policy.state_dict().items()})
    loss, pg, vf, ent = ppo_loss(pol64, obs[idx].double(), act[idx].double(), logp[idx].double(), adv[idx].double(),
                                 ret[idx].double(), agent.clip, agent.ent_coef)
    loss.backward()
    pg, vf = float(pg.detach()), float(vf.detach())
    want = _flat_grads(pol64)
    err = (g.double() - want).abs().max().item()
    bound = 1e-5 * want.abs().max().item() + 1e-7
    print("shape %s n %d count %d perm %s: err %.3e bound %.3e stats %s" % (shape, n, count, with_perm, err, bound, stats))
    assert torch.isfinite(g).all()
    assert err <= bound, (err, bound)
    assert abs(-stats[0] - pg) < 1e-4 * max(1.0, abs(pg)) and abs(0.5 * stats[1] - vf) < 1e-4 * max(1.0, vf)
    if count >= 64:
        assert 0.0 < stats[2] < 1.0                           # some ratios were clipped, not all
    assert stats[3] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(30, 32, 16), (7, 20, 10)], ids=_ids)   # an MFMA shape; a tiled one whose forward is the generic kernel
def test_null_perm_and_null_moments_equal_their_explicit_forms(shape):
    """The two argument forms only the stand-alone entry point sends through the kernels it shares with the population's:
    perm = NULL is perm = arange, and lr = 0 with NULL moments is lr = 0 with moments -- the same bits, params untouched."""
    dev = torch.device("cuda:0")
    D, h1, h2 = shape
    n, start, count = 777, 1, 700
    n_params = 2 * _n_net(D, h1, h2) + 1
    obs, act, logp, adv, ret = _rollout_like(n, D, dev, 17)
    params = (0.2 * torch.randn(n_params, generator=torch.Generator().manual_seed(3))).to(dev)
    before = params.clone()
    scratch = torch.empty(lib().pcc_ppo_scratch_floats(D, h1, h2), device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(perm, m, v):
        g, stats = torch.full((n_params,), float("nan"), device=dev), torch.full((4,), float("nan"), device=dev)
        rc = lib().pcc_ppo_minibatch_step(_p(obs), _p(act.reshape(n)), _p(logp), _p(adv), _p(ret), _p(perm), start, count, D, h1, h2,
                                          _p(params), _p(m), _p(v), 1, 0.0, 0.9, 0.999, 1e-5, 0.2, 0.01, _p(scratch), _p(g), _p(stats), st)
        torch.cuda.synchronize()
        return rc, g, stats
    rc1, g1, s1 = call(None, None, None)
    m, v = torch.zeros(n_params, device=dev), torch.zeros(n_params, device=dev)
    rc2, g2, s2 = call(torch.arange(n, device=dev), m, v)
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(g1, g2) and torch.equal(s1, s2)
    assert torch.isfinite(g1).all() and g1.abs().max() > 0
    assert torch.equal(params, before)
    assert not m.any() and not v.any()                        # lr = 0: the moments are not touched either


@pytest.mark.gpu
@pytest.mark.parametrize("n,count", [(5000, 3333), (70000, 70000)])   # (70 000: more tiles than the capped grid takes at once)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gradient_is_deterministic(shape, n, count):
    dev = torch.device("cuda:0")
    agent = _agent(shape, dev)
    obs, act, logp, adv, ret = _minibatch(agent, shape, n, dev)
    perm = torch.randperm(n, device=dev)
    g1, g2 = torch.zeros_like(agent.flat), torch.full_like(agent.flat, 3.0)
    agent.minibatch_step_fused(obs, act.reshape(n), logp, adv, ret, perm, 0, count, lr=0.0, grad_out=g1)
    s1 = agent.stats_buf.clone()
    agent.scratch.fill_(float("nan"))                         # nothing of an earlier call is read
    agent.minibatch_step_fused(obs, act.reshape(n), logp, adv, ret, perm, 0, count, lr=0.0, grad_out=g2)
    assert torch.equal(g1, g2) and torch.equal(s1, agent.stats_buf)
    assert g1.abs().max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(36, 64, 32), (120, 64, 64)], ids=_ids)
def test_optimiser_steps_match_torch_adam(shape):
    """Three consecutive fused steps against autograd + torch.optim.Adam from the same start on the same minibatches."""
    dev = torch.device("cuda:0")
    D, h1, h2 = shape
    agent = _agent(shape, dev, seed=7)
    ref = MlpPolicy(D, 1, (h1, h2)).to(dev)
    ref.load_state_dict(agent.policy.state_dict())
    opt = torch.optim.Adam(ref.parameters(), lr=agent.lr, eps=agent.adam_eps)
    n = 4096
    obs, act, logp, adv, ret = _rollout_like(n, D, dev, 3)
    with torch.no_grad():
        logp = ref.dist(obs).log_prob(act).sum(-1) + 0.1 * torch.randn(n, device=dev)
    for k in range(3):
        agent.minibatch_step_fused(obs, act.reshape(n), logp, adv, ret, None, 1000 * k, 1500)
        sl = slice(1000 * k, 1000 * k + 1500)
        loss = ppo_loss(ref, obs[sl], act[sl], logp[sl], adv[sl], ret[sl], agent.clip, agent.ent_coef)[0]
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    assert agent.adam_t == 3
    print("shape %s: max parameter difference %.3e" % (shape, (agent.flat - ref.flat_params()).abs().max().item()))
    assert torch.allclose(agent.flat, ref.flat_params(), atol=2e-5), (agent.flat - ref.flat_params()).abs().max()
    assert not torch.allclose(agent.flat, MlpPolicy(D, 1, (h1, h2)).to(dev).flat_params(), atol=1e-3)
    o = torch.randn(16, D, device=dev)                         # the module reads the updated weights (views of the flat tensor)
    assert torch.allclose(agent.policy.pi(o), ref.pi(o), atol=1e-4)
    for prm in agent.policy.parameters():
        lo, hi = agent.flat.data_ptr(), agent.flat.data_ptr() + 4 * agent.flat.numel()
        assert lo <= prm.data_ptr() < hi


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [5000, 1, 257])
@pytest.mark.parametrize("shape", SHAPES + [(33, 32, 16)], ids=_ids)
def test_forward_matches_the_framework_path(shape, rows):
    """pcc_policy_act against torch's fp32 evaluation of the same networks, the tolerances of tests/test_ppo.py."""
    torch.manual_seed(1)
    dev = torch.device("cuda:0")
    D, h1, h2 = shape
    pol = MlpPolicy(D, 1, (h1, h2)).to(dev)
    with torch.no_grad():
        pol.log_std.fill_(-0.7)
    obs = torch.randn(rows, D, device=dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        a, logp, v = pol.act_fused(obs, stochastic=False)
        a2, logp2, v2 = pol.act_fused(obs, stochastic=True)
    mu = pol.pi(obs).detach()
    print("shape %s rows %d: mean err %.3e value err %.3e" % (shape, rows, (a - mu).abs().max().item(),
                                                              (v - pol.value(obs).detach()).abs().max().item()))
    assert a.shape == (rows, 1) and torch.allclose(a, mu, atol=1e-5)
    assert torch.allclose(v, pol.value(obs).detach(), atol=1e-5)
    d = pol.dist(obs)
    assert torch.allclose(logp, d.log_prob(mu).sum(-1).detach(), atol=1e-5)
    assert torch.allclose(logp2, d.log_prob(a2).sum(-1).detach(), atol=1e-4)
    assert torch.equal(v2, v)
    if rows == 5000:
        z = (a2 - mu) / pol.log_std.exp()
        assert abs(float(z.mean())) < 0.06 and abs(float(z.std()) - 1.0) < 0.06      # standard-normal draws
    # the four outputs straight through the C ABI, mean_out included
    outs = [torch.full((rows,), float("nan"), device=dev) for _ in range(4)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib().pcc_policy_act(p(obs), rows, D, p(pol.flat_params()), h1, h2, None, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]),
                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    assert torch.equal(outs[0], a.reshape(-1)) and torch.equal(outs[1], outs[0]) and torch.equal(outs[3], v)


def _env36(n, seed, **kw):
    return pcc_rl_amd.BatchedNetworkEnv(n, device="cuda", seed=seed, history_len=3, features=list(pcc_rl_amd.METRIC_NAMES), **kw)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_ppo_arch_64_32_on_36_observations_runs_fused():
    """PPO(arch=(64, 32)) on history 3 x 12 features: fused, no RuntimeWarning, and one update() equals the framework path's
    within the three-step bound of the optimiser test scaled by the number of steps (2e-5 x steps / 3)."""
    def run(fused):
        env = _env36(2048, 41)
        assert env.obs_dim == 36
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            agent = PPO(env, arch=(64, 32), horizon=8, seed=2, epochs=2, minibatch=4096, fused_update=fused)
            assert agent.fused_update == fused
            batch = agent.collect()
            torch.manual_seed(123)
            stats = agent.update(*batch[:5])
        flat = agent.policy.flat_params().clone()
        steps = agent.adam_t if fused else None
        env.close()
        return flat, steps, stats
    a, steps, sa = run(True)
    b, _, sb = run(False)
    assert steps == 8 and steps <= 16                       # 2 epochs x 16 384 samples / 4096
    diff = (a - b).abs().max().item()
    print("PPO (36; 64, 32): %d steps, max parameter difference %.3e, stats %s / %s" % (steps, diff, sa, sb))
    assert diff <= 2e-5 * steps / 3.0, diff
    assert all(torch.isfinite(torch.tensor(list(sa.values()))))


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_ppo_policy_in_step_with_a_new_shape():
    """policy_in_step=True (pcc_rollout) works for (36; 64, 32) and collects what the policy kernel + step_into loop collects."""
    def run(in_step):
        env = _env36(4096, 43, max_steps=20)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            agent = PPO(env, arch=(64, 32), horizon=30, seed=3, policy_in_step=in_step)
            out = agent.collect()
        torch.cuda.synchronize()
        env.close()
        return out
    for x, y in zip(run(True), run(False)):
        assert torch.equal(x, y)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _rollout_against_loop(make, T, arch):
    """tests/test_rollout.py's comparison: pcc_rollout on one handle against pcc_policy_act + pcc_step on a second."""
    COLS = native.PCC_STEP_COLS
    a, r = make(), make()
    a.reset()
    r.reset()
    N, S, D = a.n_envs, a.n_senders, a.obs_dim
    torch.manual_seed(1)
    pol = MlpPolicy(D, 1, arch)
    with torch.no_grad():
        pol.log_std.fill_(-0.7)
    params = pol.flat_params().to("cuda")
    noise = torch.randn((T, N, S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    f = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    bufs = [dict(obs=f(T + 1, N, S, D), act=f(T, N, S), logp=f(T, N, S), val=f(T, N, S), rew=f(T, N, S),
                 done=torch.full((T, N), 7, dtype=torch.uint8, device="cuda"), steps=f(T, N, S, COLS).double()) for _ in range(2)]
    ba, br = bufs
    ba["obs"][0].copy_(a._obs)
    br["obs"][0].copy_(r._obs)
    a.rollout(params, noise, ba["obs"], ba["act"], ba["logp"], ba["val"], ba["rew"], ba["done"], ba["steps"], arch=arch)
    L, st = lib(), r._stream()
    for t in range(T):
        rc = L.pcc_policy_act(_p(br["obs"][t]), N * S, D, _p(params), arch[0], arch[1], _p(noise[t]), None, _p(br["act"][t]),
                              _p(br["logp"][t]), _p(br["val"][t]), st)
        assert rc == 0
        native.check(L.pcc_step(r._h, _p(br["act"][t]), 0, _p(br["obs"][t + 1]), _p(br["rew"][t]), _p(br["done"][t]),
                                _p(br["steps"][t]), 1 if r.auto_reset else 0, st))
    torch.cuda.synchronize()
    a.check_flags()
    r.check_flags()
    for k in ("obs", "act", "logp", "val", "rew", "done", "steps"):
        assert torch.equal(ba[k], br[k]), k
    assert torch.isfinite(ba["act"]).all() and torch.isfinite(ba["obs"]).all()
    done = ba["done"].bool()
    a.close()
    r.close()
    return done


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_with_a_new_shape_full_size():
    done = _rollout_against_loop(lambda: _env36(16384, 51, max_steps=15), 24, (64, 32))   # an episode boundary inside
    assert done[14].all() and not done[13].any()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_rollout_with_a_new_shape_small_batch(monkeypatch):
    monkeypatch.setattr(pcc_rl_amd.BatchedNetworkEnv, "DEFAULT_LIST_MIN_ENVS", None)   # the library's own threshold
    done = _rollout_against_loop(lambda: _env36(1000, 52, max_steps=15), 24, (64, 32))
    assert done[14].all() and not done[13].any()
    done = _rollout_against_loop(lambda: pcc_rl_amd.BatchedNetworkEnv(1000, device="cuda", seed=53, max_steps=15, history_len=10,
                                                                      features=list(pcc_rl_amd.METRIC_NAMES)), 20, (64, 64))
    assert done[14].all()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_arch_32_16_at_a_length_without_a_fixed_kernel():
    """21 observations with --arch 32,16: forward and update are fused and PPO collects with the policy kernel + step_into loop;
    pcc_rollout alone keeps refusing the length (tests/test_rollout.py pins that), before anything is stepped."""
    from pcc_rl_amd.native import PccError
    env = pcc_rl_amd.BatchedNetworkEnv(512, device="cuda", seed=61, history_len=7)
    assert env.obs_dim == 21
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        agent = PPO(env, horizon=6, seed=1, minibatch=2048)
        assert agent.fused_update
        batch = agent.collect()
        stats = agent.update(*batch[:5])
    assert all(torch.isfinite(torch.tensor(list(stats.values()))))
    obs_b = torch.zeros((3, 512, 1, 21), device="cuda")
    obs_b[0].copy_(env._obs)
    with pytest.raises(PccError, match="observation length 21"):
        env.rollout(agent.policy.flat_params(), None, obs_b, None, None, None, None, None)
    env.close()
