"""On-device PPO for the batched env.

The counterpart of the reference's training script (src/gym/stable_solve.py:39-58): the same
policy shape (separate pi / vf MLPs, hidden sizes --arch = 32,16, tanh), gamma 0.99, a constant
learning-rate schedule and an optimiser minibatch of 2048, with PPO1's other defaults (clip 0.2,
entropy coefficient 0.01, 4 epochs, step size 1e-3, lambda 0.95).  The reference collects 8192
steps from ONE env per iteration; here an iteration is T steps of N envs, everything -- rollout
buffers, advantage estimation, updates -- lives on the GPU and the env never leaves it.

This is a caller of the hot path, not part of it: stable-baselines is not available in this
image, so there is nothing to check agent-level parity against.  What is
checked (tests/test_ppo.py): the GAE recursion and the clipped objective against plain loops (CPU
tests); on the GPU the HIP kernels of the fused path -- policy forward (pcc_policy.hip), the
fp32-MFMA gradient kernel and the Adam step (pcc_ppo.hip: pcc_ppo_minibatch_step), the GAE kernel
-- against float64 autograd, torch.optim.Adam and the loop, for the reference's shape and (tests/test_ppo_shapes.py) for other
--arch and observation lengths of the library's domain (pcc_ppo_supported: csrc/pcc_mlp_tiles.h); that a short run on the GPU improves
the return; and what the whole loop costs next to the env alone (tools/ppo_throughput.py,
profiles/r04_v2_ppo_throughput.json).
"""
import ctypes
import math

import torch
from torch import nn

from .env import _ptr


class AlignedLinear(nn.Linear):
    """nn.Linear whose forward reads weight and bias from 64-byte aligned memory.  After MlpPolicy.share_flat() the parameters
    are views into ONE flat block at the offsets of the packed layout, and the CPU BLAS result for an operand at another
    alignment can differ in the last bits (the 16-wide output layer of vf, 8 bytes off a 16-byte boundary, on AMD EPYC): a
    misaligned parameter is read through an aligned copy, so moving the parameters never changes what the policy computes.
    (On the GPU the forward is nn.Linear's as it was.)"""

    def forward(self, x):
        w, b = self.weight, self.bias
        if not torch.jit.is_scripting() and w.device.type == "cpu":
            if w.data_ptr() % 64:
                w = w.clone()
            if b is not None and b.data_ptr() % 64:
                b = b.clone()
        return nn.functional.linear(x, w, b)


def mlp(inp, hidden, out):
    layers, last = [], inp
    for h in hidden:
        layers += [AlignedLinear(last, h), nn.Tanh()]
        last = h
    layers.append(AlignedLinear(last, out))
    return nn.Sequential(*layers)


_warned = set()


def _warn_once(msg):
    """A fallback off the HIP kernels of this caller is never silent (once per message and process)."""
    if msg not in _warned:
        _warned.add(msg)
        import warnings
        warnings.warn("pcc_rl_amd.ppo: " + msg, RuntimeWarning, stacklevel=3)


class MlpPolicy(nn.Module):
    """pi and vf networks of src/gym/stable_solve.py:39-45 (net_arch = [dict(pi=arch, vf=arch)])
    with a state-independent log-std, as stable-baselines' diagonal Gaussian head."""

    def __init__(self, obs_dim, act_dim=1, arch=(32, 16)):
        super().__init__()
        self.pi = mlp(obs_dim, arch, act_dim)
        self.vf = mlp(obs_dim, arch, 1)
        self.log_std = nn.Parameter(torch.zeros(act_dim))

    def dist(self, obs):
        return torch.distributions.Normal(self.pi(obs), self.log_std.exp())

    def value(self, obs):
        return self.vf(obs).squeeze(-1)

    @torch.no_grad()
    def act(self, obs, stochastic=True):
        d = self.dist(obs)
        a = d.sample() if stochastic else d.mean
        return a, d.log_prob(a).sum(-1), self.value(obs)

    def flat_params(self):
        """The parameter block pcc_policy_act reads (include/pcc_policy.h): pi {W1, b1, W2, b2, W3, b3, log_std}, vf {...}."""
        def net(seq):
            return [p.detach().reshape(-1) for m in seq if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]
        return torch.cat(net(self.pi) + [self.log_std.detach().reshape(-1)] + net(self.vf)).float().contiguous()

    def share_flat(self, into=None):
        """Move every parameter into ONE flat fp32 tensor in flat_params() order -- the module's parameters become views of
        it -- and return it: the fused optimiser step (pcc_ppo_minibatch_step) then updates the weights the framework
        path and pcc_policy_act read, with no copy in either direction.  `into`: the flat tensor to move them into (a row
        of a population's block, PopulationPPO), instead of a new one."""
        flat = self.flat_params().clone()
        if into is not None:
            with torch.no_grad():
                into.copy_(flat)
            flat = into
        off = 0

        def net(seq):
            return [p for m in seq if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]
        for prm in net(self.pi) + [self.log_std] + net(self.vf):
            n = prm.numel()
            prm.data = flat[off:off + n].view(prm.shape)
            off += n
        assert off == flat.numel()
        return flat

    @property
    def hidden(self):
        """The two hidden sizes (h1, h2) -- what the HIP library's policy kernels take -- or None when the policy is not two
        hidden layers with one action."""
        out = [m.out_features for m in self.pi if isinstance(m, nn.Linear)]
        return (out[0], out[1]) if len(out) == 3 and out[2] == 1 else None

    def fused_ok(self, obs):
        """Whether pcc_policy_act covers this policy and observation batch (two hidden layers, one action, fp32 on the GPU)."""
        return self.hidden is not None and obs.is_cuda and obs.dtype == torch.float32

    @torch.no_grad()
    def act_fused(self, obs, stochastic=True, params=None, noise=None, out=None):
        """act() as ONE kernel launch of the HIP library; returns (action [N, 1], log-probability [N], value [N]) like act().
        A rollout loop passes `params` (flat_params(), built once per rollout -- it is a 13-tensor torch.cat), its own
        `noise` row and `out` = (action, logp, value) rows of its buffers, so that a step adds no framework launch."""
        from .native import lib
        if not self.fused_ok(obs):
            _warn_once("the policy forward runs on the framework path (no pcc_policy_act for this policy / observation batch)")
            return self.act(obs, stochastic)
        h1, h2 = self.hidden
        n, D = obs.shape
        if params is None:
            params = self.flat_params()
        if noise is None and stochastic:
            noise = torch.randn(n, device=obs.device)
        if out is None:
            a = torch.empty(n, device=obs.device)
            logp, v = torch.empty_like(a), torch.empty_like(a)
        else:
            a, logp, v = out
        rc = lib().pcc_policy_act(_ptr(obs.contiguous()), n, D, _ptr(params), h1, h2,
                                  _ptr(noise if stochastic else None), None, _ptr(a), _ptr(logp), _ptr(v),
                                  ctypes.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
        if rc != 0:   # a shape outside the library's domain (include/pcc_policy.h: pcc_ppo_supported)
            _warn_once("pcc_policy_act has no kernel for %d observations x hidden %d-%d: the policy forward runs on the framework "
                       "path (several times slower)" % (D, h1, h2))
            a2, logp2, v2 = self.act(obs, stochastic)
            if out is not None:
                a.copy_(a2.reshape(-1)); logp.copy_(logp2); v.copy_(v2)
            return a2, logp2, v2
        return a.reshape(n, 1), logp, v


def gae(rewards, values, dones, last_value, gamma=0.99, lam=0.95):
    """Generalised advantage estimation over [T, N] tensors.  dones[t] marks that the env was reset
    after step t (the next observation belongs to a new episode)."""
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    running = torch.zeros_like(last_value)
    next_value = last_value
    for t in range(T - 1, -1, -1):
        alive = 1.0 - dones[t].to(rewards.dtype)
        delta = rewards[t] + gamma * next_value * alive - values[t]
        running = delta + gamma * lam * alive * running
        adv[t] = running
        next_value = values[t]
    return adv, adv + values


def gae_fused(rewards, values, dones, last_value, gamma=0.99, lam=0.95):
    """gae() as one launch of the HIP library (pcc_gae: thread = env, T steps backwards) for fp32 [T, N] rows on the GPU."""
    from .native import lib
    if not (rewards.is_cuda and rewards.dtype == torch.float32 and rewards.dim() == 2):
        return gae(rewards, values, dones, last_value, gamma, lam)
    T, N = rewards.shape
    rewards, values, last_value = rewards.contiguous(), values.contiguous(), last_value.contiguous().float()
    d8 = dones.contiguous().view(torch.uint8) if dones.dtype == torch.bool else dones.to(torch.uint8).contiguous()
    adv, ret = torch.empty_like(rewards), torch.empty_like(rewards)
    rc = lib().pcc_gae(_ptr(rewards), _ptr(values), _ptr(d8), _ptr(last_value), T, N, gamma, lam, _ptr(adv), _ptr(ret),
                       ctypes.c_void_p(torch.cuda.current_stream(rewards.device).cuda_stream))
    if rc != 0:
        raise RuntimeError("pcc_gae failed (%d)" % rc)
    return adv, ret


def ppo_loss(policy, obs, act, logp_old, adv, ret, clip=0.2, ent_coef=0.01):
    """PPO1's objective on one minibatch: clipped surrogate + 0.5 * value error - ent_coef * entropy.
    Returns (loss, policy term, value term, entropy)."""
    d = policy.dist(obs)
    logp = d.log_prob(act).sum(-1)
    ratio = (logp - logp_old).exp()
    pg = -torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean()
    vf = 0.5 * (policy.value(obs) - ret).pow(2).mean()
    ent = d.entropy().sum(-1).mean()
    return pg + vf - ent_coef * ent, pg, vf, ent


def _refuse_normalize(normalize_obs, policy_in_step, env):
    """normalize_obs needs the rows between the env and the policy: not with the policy inside the env's launches."""
    if not normalize_obs:
        return
    if policy_in_step:
        raise ValueError("normalize_obs=True cannot be combined with policy_in_step=True: the policy inside the env's launches "
                         "(pcc_rollout) reads the raw observation rows, not the normalised ones")
    if hasattr(env, "groups"):
        raise ValueError("normalize_obs=True is not supported over a GroupedNetworkEnv: its groups are stepped on their own streams "
                         "and the policy reads the raw observation rows there")


def _check_normalize(sd, normalize_obs):
    if bool(sd.get("normalize_obs", False)) != bool(normalize_obs):
        raise ValueError("the checkpoint was written with normalize_obs=%s, this object has normalize_obs=%s: weights without "
                         "their normaliser are meaningless" % (bool(sd.get("normalize_obs", False)), bool(normalize_obs)))


class PPO(object):
    def __init__(self, env, arch=(32, 16), gamma=0.99, lam=0.95, clip=0.2, ent_coef=0.01, lr=1e-3,
                 epochs=4, minibatch=None, horizon=64, seed=0, fused_update=True, policy_in_step=False,
                 normalize_obs=False, clip_obs=10.0, norm_eps=1e-8):
        """minibatch None = a quarter of the rollout, at least 2048: the reference's ratio (optim_batchsize 2048 of a
        timesteps_per_actorbatch of 8192, stable_solve.py:52) -- at 65 536 envs x 64 steps a fixed 2048 would be 2 048
        optimiser steps per epoch, thousands of launches of a few microseconds of work each.
        policy_in_step: collect() runs the horizon as ONE closed-loop library call per env (group) -- env.rollout, pcc_rollout:
        the policy inside the env's own launches -- with the same numbers, bit for bit, as the policy kernel + step_into loop.
        normalize_obs: the policy sees clamp((obs - mean) / sqrt(var + norm_eps), -clip_obs, clip_obs) with the running moments of
        the raw rows (obsnorm.ObsNormalizer): frozen during a rollout, updated once at its end."""
        if policy_in_step and torch.device(env.device).type != "cuda":
            raise ValueError("PPO(policy_in_step=True) runs the policy inside the env's HIP launches: it needs the env on the GPU "
                             "(device=%r)" % (env.device,))
        self.policy_in_step = bool(policy_in_step)
        self.normalize_obs = bool(normalize_obs)
        _refuse_normalize(self.normalize_obs, policy_in_step, env)
        self.env, self.gamma, self.lam, self.clip, self.ent_coef = env, gamma, lam, clip, ent_coef
        self.epochs, self.minibatch, self.horizon = epochs, minibatch, horizon
        torch.manual_seed(seed)
        if hasattr(env, "groups"):   # GroupedNetworkEnv: the surface of a BatchedNetworkEnv, from its groups
            env.obs_dim, env.n_senders = env.groups[0].obs_dim, env.groups[0].n_senders
        self.policy = MlpPolicy(env.obs_dim, 1, arch).to(env.device)
        if hasattr(env, "groups") and not (len(arch) == 2 and env.n_senders == 1 and torch.device(env.device).type == "cuda"):
            # (a GroupedNetworkEnv is stepped group by group on its streams by the fused rollout only: it has no step() of its own)
            raise ValueError("PPO over a GroupedNetworkEnv needs the fused rollout (a two-hidden-layer policy, one sender, on the GPU)")
        self.lr, self.adam_eps = lr, 1e-5
        # the fused optimiser step (pcc_ppo_minibatch_step: gradient + Adam in two launches) when the library has a kernel
        # for this shape; the framework path (autograd + torch.optim.Adam, the same arithmetic) otherwise
        self.fused_update = bool(fused_update) and self._fused_update_ok()
        if fused_update and not self.fused_update:
            _warn_once("PPO.update runs autograd + torch.optim.Adam (no pcc_ppo_minibatch_step for observation length %d, hidden %s, "
                       "%d sender(s) on %s): about 20x slower than the fused step" % (env.obs_dim, list(arch), env.n_senders, env.device))
        if self.fused_update:
            from .native import lib
            self.flat = self.policy.share_flat()
            self.adam_m, self.adam_v, self.adam_t = torch.zeros_like(self.flat), torch.zeros_like(self.flat), 0
            self.scratch = torch.empty(lib().pcc_ppo_scratch_floats(env.obs_dim, arch[0], arch[1]), device=env.device)
            self.stats_buf = torch.zeros(4, device=env.device)
        self.opt = torch.optim.Adam(self.policy.parameters(), lr=lr, eps=self.adam_eps)
        self.obs = env.reset().clone()
        if self.normalize_obs:
            from .obsnorm import ObsNormalizer
            self.obs_norm = ObsNormalizer(env.obs_dim, 1, clip_obs, norm_eps, device=env.device)
            self.raw_obs = self.obs
            self.obs = self.obs_norm.normalise(self.raw_obs)
        if self.minibatch is None:
            self.minibatch = max(2048, env.n_envs * horizon // 4)

    def _fused_update_ok(self):
        env = self.env
        hidden = self.policy.hidden
        if not (torch.device(env.device).type == "cuda" and hidden is not None and env.n_senders == 1):
            return False
        from .native import lib
        return lib().pcc_ppo_supported(int(env.obs_dim), hidden[0], hidden[1]) == 1

    def collect(self):
        """One rollout of `horizon` steps of every env.  The policy kernel reads the observation row the env wrote and
        writes action / log-probability / value into the rollout rows; the env reads that action row and writes the next
        observation, reward and done rows: two library calls and three kernels per step, no framework launch, no copy."""
        env, T, N = self.env, self.horizon, self.env.n_envs
        dev = env.device
        obs_b = torch.empty((T + 1, N, env.obs_dim), device=dev)   # row t: what the policy saw at step t; row T: the last
        act_b = torch.empty((T, N, 1), device=dev)
        logp_b = torch.empty((T, N), device=dev)
        val_b = torch.empty((T, N), device=dev)
        rew_b = torch.empty((T, N), device=dev)
        done_b = torch.empty((T, N), dtype=torch.bool, device=dev)
        if self.normalize_obs:
            # the env writes raw rows; after each step ONE normalise launch fills the row the policy reads.  The statistics are
            # frozen during the rollout: logp_old, the values and the update all see the same inputs.
            norm = self.obs_norm
            raw_b = torch.empty((T + 1, N, env.obs_dim), device=dev)
            raw_b[0] = self.raw_obs
            norm.normalise(raw_b[0], obs_b[0])
        else:
            obs_b[0] = self.obs
        fused = self.policy.fused_ok(obs_b[0]) and env.n_senders == 1
        groups = getattr(env, "groups", None)
        if self.policy_in_step and not fused:
            raise ValueError("PPO(policy_in_step=True) needs the fused rollout: a two-hidden-layer policy, one sender, on the GPU")
        if self.policy_in_step:
            # the whole horizon as one pcc_rollout per env (group): the same noise, parameters and rows as the loop below
            arch = self.policy.hidden
            params = self.policy.flat_params()
            noise = torch.randn((T, N), device=dev)
            u8 = done_b.view(torch.uint8)
            if groups is None:
                env.rollout(params, noise, obs_b, act_b, logp_b, val_b, rew_b, u8, arch=arch)
            else:
                n = env.group_size
                cur = torch.cuda.current_stream(dev)
                # (a group's rows of [T(+1), N] buffers are strided: each group fills contiguous buffers of its own on its stream)
                parts = []
                for g, eg in enumerate(groups):
                    lo, hi = g * n, (g + 1) * n
                    env.streams[g].wait_stream(cur)
                    with torch.cuda.stream(env.streams[g]):
                        ob = torch.empty((T + 1, n, env.obs_dim), device=dev)
                        ob[0] = obs_b[0, lo:hi]
                        bufs = (torch.empty((T, n, 1), device=dev), torch.empty((T, n), device=dev), torch.empty((T, n), device=dev),
                                torch.empty((T, n), device=dev), torch.empty((T, n), dtype=torch.uint8, device=dev))
                        eg.rollout(params, noise[:, lo:hi].contiguous(), ob, *bufs, arch=arch)
                        parts.append((lo, hi, ob, bufs))
                for g, (lo, hi, ob, bufs) in enumerate(parts):
                    cur.wait_stream(env.streams[g])
                    obs_b[1:, lo:hi] = ob[1:]
                    for dst, src in zip((act_b, logp_b, val_b, rew_b, u8), bufs):
                        dst[:, lo:hi] = src
                    for tns in (ob,) + bufs:
                        tns.record_stream(cur)
        elif fused and groups is not None:
            # Double-buffered sampling (GroupedNetworkEnv: the same envs as G groups on their own streams): group g's
            # policy kernel and env step are queued on stream g, nothing joins the groups inside the rollout -- while one
            # group's env launches run out their tails (a third of the wavefront slots busy), the
            # other group's policy kernel and launches fill the machine.  Same numbers as one batch: a group holds the
            # global env ids g * n .. and reads its own rows of every buffer.
            params = self.policy.flat_params()
            noise = torch.randn((T, N), device=dev)
            n = env.group_size
            cur = torch.cuda.current_stream(dev)
            for s in env.streams:
                s.wait_stream(cur)                                 # the buffers and the noise were made on this stream
            for t in range(T):
                for g, eg in enumerate(groups):
                    lo, hi = g * n, (g + 1) * n
                    with torch.cuda.stream(env.streams[g]):
                        self.policy.act_fused(obs_b[t, lo:hi], True, params, noise[t, lo:hi],
                                              (act_b[t, lo:hi].reshape(n), logp_b[t, lo:hi], val_b[t, lo:hi]))
                        eg.step_into(act_b[t, lo:hi], obs_b[t + 1, lo:hi], rew_b[t, lo:hi], done_b[t, lo:hi])
            for s in env.streams:
                cur.wait_stream(s)
        elif fused:
            params = self.policy.flat_params()                     # once per rollout, not per step
            noise = torch.randn((T, N), device=dev)                # the horizon's draws in one launch
            for t in range(T):
                self.policy.act_fused(obs_b[t], True, params, noise[t], (act_b[t].reshape(N), logp_b[t], val_b[t]))
                if self.normalize_obs:
                    env.step_into(act_b[t], raw_b[t + 1], rew_b[t], done_b[t])
                    norm.normalise(raw_b[t + 1], obs_b[t + 1])
                else:
                    env.step_into(act_b[t], obs_b[t + 1], rew_b[t], done_b[t])   # tensors in, tensors out, no host round trip
        else:
            for t in range(T):
                a, logp, v = self.policy.act(obs_b[t])
                act_b[t], logp_b[t], val_b[t] = a, logp, v
                nobs, r, d, _ = env.step(a)
                if self.normalize_obs:
                    raw_b[t + 1] = nobs
                    norm.normalise(raw_b[t + 1], obs_b[t + 1])
                else:
                    obs_b[t + 1] = nobs
                rew_b[t], done_b[t] = r, d
        obs = obs_b[T]
        self.obs = obs.clone()
        if self.normalize_obs:
            self.raw_b, self.raw_obs = raw_b, raw_b[T].clone()
            norm.update(raw_b[:T])   # rows 0 .. T - 1: what the policy saw
        obs_b = obs_b[:T]
        with torch.no_grad():
            last_v = self.policy.value(obs)
        # never train on corrupted rollouts: an overflowed in-flight ring / an empty ring pool (a trained
        # policy can push many deep-queue envs to MAX_RATE: BatchedNetworkEnv(ring_pools=...)) is flagged, not silent
        env.check_flags()
        adv, ret = (gae_fused if fused else gae)(rew_b, val_b, done_b, last_v, self.gamma, self.lam)
        return obs_b, act_b, logp_b, adv, ret, rew_b

    def update(self, obs_b, act_b, logp_b, adv, ret):
        n = obs_b.shape[0] * obs_b.shape[1]
        obs_f, act_f = obs_b.reshape(n, -1), act_b.reshape(n, -1)
        logp_f, adv_f, ret_f = logp_b.reshape(n), adv.reshape(n), ret.reshape(n)
        adv_f = (adv_f - adv_f.mean()) / (adv_f.std() + 1e-8)
        if self.fused_update:
            return self._update_fused(obs_f, act_f, logp_f, adv_f, ret_f)
        stats = {}
        for _ in range(self.epochs):
            perm = torch.randperm(n, device=obs_f.device)
            for i in range(0, n, self.minibatch):
                idx = perm[i:i + self.minibatch]
                loss, pg, vf, ent = ppo_loss(self.policy, obs_f[idx], act_f[idx], logp_f[idx], adv_f[idx], ret_f[idx],
                                             self.clip, self.ent_coef)
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                self.opt.step()
                stats = {"pg": pg.detach(), "vf": vf.detach(), "entropy": ent.detach()}
        return {k: float(v) for k, v in stats.items()}

    def minibatch_step_fused(self, obs_f, act_f, logp_f, adv_f, ret_f, perm, start, count, lr=None, grad_out=None):
        """One optimiser step on samples perm[start : start + count] of the flattened rollout as two launches of the HIP
        library (include/pcc_policy.h: pcc_ppo_minibatch_step).  lr=0: gradient only (into grad_out)."""
        from .native import lib
        lr = self.lr if lr is None else lr
        if start < 0 or count < 1 or start + count > (perm.numel() if perm is not None else obs_f.shape[0]):
            raise ValueError("minibatch [%d, %d) outside the rollout" % (start, start + count))
        if lr != 0.0:
            self.adam_t += 1
        D = obs_f.shape[1]
        h1, h2 = self.policy.hidden
        rc = lib().pcc_ppo_minibatch_step(_ptr(obs_f), _ptr(act_f), _ptr(logp_f), _ptr(adv_f), _ptr(ret_f), _ptr(perm), start, count,
                                          D, h1, h2, _ptr(self.flat), _ptr(self.adam_m), _ptr(self.adam_v), max(self.adam_t, 1),
                                          lr, 0.9, 0.999, self.adam_eps, self.clip, self.ent_coef, _ptr(self.scratch),
                                          _ptr(grad_out), _ptr(self.stats_buf),
                                          ctypes.c_void_p(torch.cuda.current_stream(obs_f.device).cuda_stream))
        if rc != 0:
            raise RuntimeError("pcc_ppo_minibatch_step failed (%d)" % rc)

    def _update_fused(self, obs_f, act_f, logp_f, adv_f, ret_f):
        n = obs_f.shape[0]
        obs_f, act_f = obs_f.contiguous(), act_f.reshape(n).contiguous()
        logp_f, adv_f, ret_f = logp_f.contiguous(), adv_f.contiguous(), ret_f.contiguous()
        for _ in range(self.epochs):
            perm = torch.randperm(n, device=obs_f.device)
            for i in range(0, n, self.minibatch):
                self.minibatch_step_fused(obs_f, act_f, logp_f, adv_f, ret_f, perm, i, min(self.minibatch, n - i))
        st = self.stats_buf.tolist()   # of the last minibatch, like the framework path
        ent = float(self.policy.log_std.detach().sum()) + 0.5 * (1.0 + math.log(2.0 * math.pi)) * self.policy.log_std.numel()
        return {"pg": -st[0], "vf": 0.5 * st[1], "entropy": ent, "clip_frac": st[2]}

    def state_dict(self):
        """Everything the next iterate() depends on, for a checkpoint that resumes bit for bit: the parameters and Adam's state (the
        flat block with m, v, t on the fused path, the module's and the torch optimiser's state_dict on the framework path), the
        observation the next rollout starts from, torch's CPU and device generator states (the rollout's noise and the
        minibatch permutations come from the device's), and the env's snapshot (BatchedNetworkEnv.snapshot: not with the env options it
        refuses).  torch.save() takes it as it is."""
        dev = torch.device(self.env.device)
        sd = {"format": 1, "fused_update": self.fused_update, "obs_dim": int(self.env.obs_dim), "n_envs": int(self.env.n_envs),
              "obs": self.obs.detach().clone(), "torch_rng": torch.get_rng_state(),
              "device_rng": torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None, "env": self.env.snapshot()}
        if self.fused_update:
            sd.update(flat=self.flat.detach().clone(), adam_m=self.adam_m.clone(), adam_v=self.adam_v.clone(), adam_t=int(self.adam_t))
        else:
            sd.update(policy={k: v.detach().clone() for k, v in self.policy.state_dict().items()}, opt=self.opt.state_dict())
        if self.normalize_obs:   # (without it the keys are what they were)
            sd.update(normalize_obs=True, obs_norm=self.obs_norm.state_dict(), raw_obs=self.raw_obs.detach().clone())
        return sd

    def load_state_dict(self, sd):
        """Continue from a state_dict() of a PPO of the same construction (env configuration, arch, update path): the env is restored
        from its snapshot (it must have been reset once: the constructor did that), then the parameters, the optimiser, the
        observation and the generator states."""
        dev = torch.device(self.env.device)
        if sd.get("format") != 1:
            raise ValueError("not a PPO.state_dict() of this version")
        if bool(sd["fused_update"]) != self.fused_update or sd["obs_dim"] != int(self.env.obs_dim) or sd["n_envs"] != int(self.env.n_envs):
            raise ValueError("the checkpoint is of another PPO: fused_update=%s, obs_dim=%d, n_envs=%d; this one: %s, %d, %d"
                             % (sd["fused_update"], sd["obs_dim"], sd["n_envs"], self.fused_update, self.env.obs_dim, self.env.n_envs))
        _check_normalize(sd, self.normalize_obs)
        if self.fused_update and sd["flat"].numel() != self.flat.numel():
            raise ValueError("the checkpoint's policy has %d parameters, this one %d (another --arch)" % (sd["flat"].numel(), self.flat.numel()))
        self.env.restore(sd["env"])
        if self.fused_update:
            with torch.no_grad():
                self.flat.copy_(sd["flat"])   # (the module's parameters are views of it: share_flat)
                self.adam_m.copy_(sd["adam_m"])
                self.adam_v.copy_(sd["adam_v"])
            self.adam_t = int(sd["adam_t"])
        else:
            self.policy.load_state_dict(sd["policy"])
            self.opt.load_state_dict(sd["opt"])
        self.obs = sd["obs"].to(dev).clone()
        if self.normalize_obs:
            self.obs_norm.load_state_dict(sd["obs_norm"])
            self.raw_obs = sd["raw_obs"].to(dev).clone()
        torch.set_rng_state(sd["torch_rng"].cpu())
        if dev.type == "cuda" and sd.get("device_rng") is not None:
            torch.cuda.set_rng_state(sd["device_rng"].cpu(), dev)

    def iterate(self):
        obs_b, act_b, logp_b, adv, ret, rew = self.collect()
        stats = self.update(obs_b, act_b, logp_b, adv, ret)
        stats["mean_step_reward"] = float(rew.mean())
        return stats


# ------------------------------------------------------------------------------------------------------------ population
def population_sample_index(member, t, env, n_envs, n_members):
    """The index of member `member`'s sample (step t, its env `env`) in the flattened [T * n_envs] rollout arrays every member
    shares: member m owns the envs m * n_envs / n_members ... of each row (include/pcc_policy.h).  Integers or tensors."""
    n_m = n_envs // n_members
    return t * n_envs + member * n_m + env


def population_permutations(T, n_envs, n_members, device="cpu", generator=None):
    """[n_members][T * n_m] int64: row m is a random permutation of member m's own T * n_m samples, as indices into the shared
    [T * n_envs] arrays (population_sample_index) -- what pcc_ppo_minibatch_step_pop takes as `perm`.  One draw for all members."""
    n_m = n_envs // n_members
    local = torch.rand((n_members, T * n_m), device=device, generator=generator).argsort(dim=1)   # row m: a permutation of 0 .. T n_m - 1
    member = torch.arange(n_members, device=device).unsqueeze(1)
    return population_sample_index(member, local // n_m, local % n_m, n_envs, n_members).contiguous()


def normalise_per_member(adv, n_members):
    """PPO.update's advantage normalisation, (a - mean) / (std + 1e-8), for each member over its own samples: the columns
    m * n_m ... of the [T][N] rows.  Member by member, so that no member's numbers depend on another's."""
    T, N = adv.shape
    n_m = N // n_members
    out = torch.empty_like(adv)
    for m in range(n_members):
        a = adv[:, m * n_m:(m + 1) * n_m].contiguous()   # (the sums' order does not depend on where the member's columns sit)
        out[:, m * n_m:(m + 1) * n_m] = (a - a.mean()) / (a.std() + 1e-8)
    return out


HYPER_COLS = 8   # a row of `hyper` (include/pcc_policy.h): {lr, clip, ent_coef, gamma, lam, 0, 0, 0}
HYPER_NAMES = ("lr", "clip", "ent_coef", "gamma", "lam")   # the columns PopulationPPO.evolve can perturb or bound, by name


def explore_matrix(factors=(0.8, 1.2), explore=("lr", "ent_coef"), bounds=None):
    """The [8][4] rows {factor_lo, factor_hi, min, max} pcc_pbt_evolve takes (include/pcc_policy.h), as a list: the columns
    named in `explore` get `factors`, every other column -- the three reserved ones too -- {1, 1, -inf, +inf}, which inherits
    the parent's value unchanged; bounds: {name: (lo, hi)}."""
    inf = float("inf")
    rows = [[1.0, 1.0, -inf, inf] for _ in range(HYPER_COLS)]
    lo, hi = float(factors[0]), float(factors[1])
    for name in explore:
        if name not in HYPER_NAMES:
            raise ValueError("evolve: no hyper-parameter %r (one of %s)" % (name, ", ".join(HYPER_NAMES)))
        rows[HYPER_NAMES.index(name)][:2] = [lo, hi]
    for name, b in (bounds or {}).items():
        if name not in HYPER_NAMES:
            raise ValueError("evolve: bounds for %r, which is no hyper-parameter (one of %s)" % (name, ", ".join(HYPER_NAMES)))
        rows[HYPER_NAMES.index(name)][2:] = [float(b[0]), float(b[1])]
    return rows


class PopulationPPO(object):
    """`members` independent PPO learners -- each its own policy, Adam state and hyper-parameters -- on `members` equal slices
    of ONE BatchedNetworkEnv: the env is stepped once per step for the whole batch, and the policy forward, the advantage
    estimation and the optimiser step are each one library call for all members (include/pcc_policy.h: pcc_policy_act_pop,
    pcc_gae_pop, pcc_ppo_minibatch_step_pop), bit-identical to the members run one by one through the single-policy entry
    points.  Seeds for a learning curve, or a sweep over lr / clip / ent_coef / gamma / lam: each is a scalar or one value per
    member.  Member m's policy starts as PPO(seed=seeds[m])'s: like PPO, construction reseeds torch's global generators
    (torch.manual_seed, member by member), so they are left seeded by seeds[-1], and the rollout's noise and the minibatch
    permutations are drawn from the device's from there.  There is no framework path: anything the library has no kernel
    for raises ValueError."""

    def __init__(self, env, members, arch=(32, 16), lr=1e-3, clip=0.2, ent_coef=0.01, gamma=0.99, lam=0.95, seeds=None,
                 epochs=4, minibatch=None, horizon=64, normalize_obs=False, clip_obs=10.0, norm_eps=1e-8):
        from .env import BatchedNetworkEnv
        from .native import lib
        members = int(members)
        self.normalize_obs = bool(normalize_obs)
        _refuse_normalize(self.normalize_obs, False, env)
        if members < 1 or members > 1024:
            raise ValueError("PopulationPPO: members = %d (1 .. 1024)" % members)
        if len(arch) != 2:
            raise ValueError("PopulationPPO needs a policy of two hidden layers (arch = %r)" % (tuple(arch),))
        if int(env.n_envs) % members != 0:
            raise ValueError("PopulationPPO: %d envs do not divide into %d members" % (env.n_envs, members))
        cols = []
        for name, v in (("lr", lr), ("clip", clip), ("ent_coef", ent_coef), ("gamma", gamma), ("lam", lam)):
            try:
                vals = [float(v)] * members          # a scalar: a number, a numpy scalar, a 0-dim tensor
            except (TypeError, ValueError):
                vals = [float(x) for x in v]
            if len(vals) != members:
                raise ValueError("PopulationPPO: %s has %d values for %d members" % (name, len(vals), members))
            cols.append(vals)
        seeds = list(range(members)) if seeds is None else [int(x) for x in seeds]
        if len(seeds) != members:
            raise ValueError("PopulationPPO: seeds has %d values for %d members" % (len(seeds), members))
        if not isinstance(env, BatchedNetworkEnv) or torch.device(env.device).type != "cuda" or env.n_senders != 1:
            raise ValueError("PopulationPPO needs a BatchedNetworkEnv with one sender on the GPU (no GroupedNetworkEnv)")
        if lib().pcc_ppo_supported(int(env.obs_dim), int(arch[0]), int(arch[1])) != 1:
            raise ValueError("PopulationPPO: the library has no kernels for %d observations x hidden %s (pcc_ppo_supported)"
                             % (env.obs_dim, list(arch)))
        self.env, self.members, self.arch = env, members, (int(arch[0]), int(arch[1]))
        self.epochs, self.horizon, self.adam_eps = epochs, horizon, 1e-5
        self.n_member = int(env.n_envs) // members
        dev = env.device
        self.hyper_rows = [list(r) + [0.0] * (HYPER_COLS - 5) for r in zip(*cols)]
        self.hyper = torch.tensor(self.hyper_rows, dtype=torch.float32, device=dev)
        self.generation = 0   # evolve() calls so far: the Philox counter of the next one
        D = int(env.obs_dim)
        self.n_params = 2 * (self.arch[0] * D + self.arch[0] + self.arch[1] * self.arch[0] + 2 * self.arch[1] + 1) + 1
        self.param_stride = (self.n_params + 63) // 64 * 64   # every member's block 256-byte aligned
        self.flat = torch.zeros((members, self.param_stride), device=dev)
        self.policies = []
        for m in range(members):
            torch.manual_seed(seeds[m])                         # as PPO(seed=seeds[m]) makes its policy
            pol = MlpPolicy(D, 1, self.arch).to(dev)
            pol.share_flat(into=self.flat[m, :self.n_params])
            self.policies.append(pol)
        self.adam_m, self.adam_v, self.adam_t = torch.zeros_like(self.flat), torch.zeros_like(self.flat), 0
        self.scratch_floats = lib().pcc_ppo_scratch_floats(D, *self.arch)
        self.scratch = torch.empty(members * self.scratch_floats, device=dev)
        self.stats_buf = torch.zeros((members, 4), device=dev)
        self.obs = env.reset().clone()
        if self.normalize_obs:   # every member its own moments of its own columns (obsnorm.ObsNormalizer)
            from .obsnorm import ObsNormalizer
            self.obs_norm = ObsNormalizer(D, members, clip_obs, norm_eps, device=dev)
            self.raw_obs = self.obs
            self.obs = self.obs_norm.normalise(self.raw_obs)
        per_member = self.n_member * horizon
        self.minibatch = min(per_member, max(2048, per_member // 4)) if minibatch is None else int(minibatch)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.env.device).cuda_stream)

    def _act(self, obs, noise, act, logp, val):
        """The policies on one [N, D] observation row: member m on its slice with its parameters, one launch."""
        from .native import lib
        N, D = obs.shape
        rc = lib().pcc_policy_act_pop(_ptr(obs), N, D, _ptr(self.flat), self.param_stride, self.members, self.arch[0], self.arch[1],
                                      _ptr(noise), None, _ptr(act), _ptr(logp), _ptr(val), self._stream())
        if rc != 0:
            raise RuntimeError("pcc_policy_act_pop failed (%d)" % rc)

    def _gae(self, rew_b, val_b, done_b, last_v):
        from .native import lib
        T, N = rew_b.shape
        adv, ret = torch.empty_like(rew_b), torch.empty_like(rew_b)
        d8 = done_b.view(torch.uint8)
        rc = lib().pcc_gae_pop(_ptr(rew_b), _ptr(val_b), _ptr(d8), _ptr(last_v), T, N, self.members, _ptr(self.hyper), _ptr(adv), _ptr(ret),
                               self._stream())
        if rc != 0:
            raise RuntimeError("pcc_gae_pop failed (%d)" % rc)
        return adv, ret

    def collect(self, noise=None):
        """One rollout of `horizon` steps of the whole batch: per step pcc_policy_act_pop (every member on its slice) and ONE
        env step; then the last values, the env's flags, and pcc_gae_pop with every member's gamma and lambda.  noise: the
        [horizon, n_envs] standard-normal draws (default: drawn here).  Returns PPO.collect()'s tuple; the value and done rows
        stay in self.val_b / self.done_b."""
        env, T, N = self.env, self.horizon, int(self.env.n_envs)
        dev = env.device
        obs_b = torch.empty((T + 1, N, env.obs_dim), device=dev)
        act_b = torch.empty((T, N, 1), device=dev)
        logp_b, val_b, rew_b = (torch.empty((T, N), device=dev) for _ in range(3))
        done_b = torch.empty((T, N), dtype=torch.bool, device=dev)
        if self.normalize_obs:   # as PPO.collect: raw rows from the env, one normalise launch per step, frozen statistics
            norm = self.obs_norm
            raw_b = torch.empty((T + 1, N, env.obs_dim), device=dev)
            raw_b[0] = self.raw_obs
            norm.normalise(raw_b[0], obs_b[0])
        else:
            obs_b[0] = self.obs
        if noise is None:
            noise = torch.randn((T, N), device=dev)
        for t in range(T):
            self._act(obs_b[t], noise[t], act_b[t].reshape(N), logp_b[t], val_b[t])
            if self.normalize_obs:
                env.step_into(act_b[t], raw_b[t + 1], rew_b[t], done_b[t])
                norm.normalise(raw_b[t + 1], obs_b[t + 1])
            else:
                env.step_into(act_b[t], obs_b[t + 1], rew_b[t], done_b[t])
        self.obs = obs_b[T].clone()
        if self.normalize_obs:
            self.raw_b, self.raw_obs = raw_b, raw_b[T].clone()
        last_v = torch.empty(N, device=dev)
        self._act(obs_b[T], None, None, None, last_v)
        env.check_flags()
        adv, ret = self._gae(rew_b, val_b, done_b, last_v)
        self.val_b, self.done_b = val_b, done_b
        if self.normalize_obs:
            norm.update(raw_b[:T])   # rows 0 .. T - 1: what the policies saw
        return obs_b[:T], act_b, logp_b, adv, ret, rew_b

    def normalise(self, adv):
        return normalise_per_member(adv, self.members)

    def minibatch_step(self, obs_f, act_f, logp_f, adv_f, ret_f, perm, start, count, grad_out=None):
        """One optimiser step of every member on its samples perm[m][start : start + count] (global indices into the flattened
        rollout): two launches (pcc_ppo_minibatch_step_pop)."""
        from .native import lib
        if start < 0 or count < 1 or start + count > perm.shape[1]:
            raise ValueError("minibatch [%d, %d) outside a member's rollout" % (start, start + count))
        self.adam_t += 1
        D = obs_f.shape[1]
        rc = lib().pcc_ppo_minibatch_step_pop(_ptr(obs_f), _ptr(act_f), _ptr(logp_f), _ptr(adv_f), _ptr(ret_f), _ptr(perm), perm.stride(0),
                                              start, count, D, self.arch[0], self.arch[1], _ptr(self.flat), _ptr(self.adam_m),
                                              _ptr(self.adam_v), self.param_stride, self.members, _ptr(self.hyper), self.adam_t, 0.9, 0.999,
                                              self.adam_eps, _ptr(self.scratch), _ptr(grad_out), _ptr(self.stats_buf), self._stream())
        if rc != 0:
            raise RuntimeError("pcc_ppo_minibatch_step_pop failed (%d)" % rc)

    def update(self, obs_b, act_b, logp_b, adv, ret, perms=None):
        """`epochs` passes over every member's own samples in minibatches of self.minibatch samples per member.  perms: one
        [members][T * n_m] tensor per epoch (population_permutations; default: drawn here, one draw per epoch)."""
        T, N = adv.shape
        n = T * N
        adv_f = self.normalise(adv).reshape(n)
        obs_f, act_f = obs_b.reshape(n, -1).contiguous(), act_b.reshape(n).contiguous()
        logp_f, ret_f = logp_b.reshape(n).contiguous(), ret.reshape(n).contiguous()
        per_member = T * self.n_member
        for e in range(self.epochs):
            perm = perms[e] if perms is not None else population_permutations(T, N, self.members, device=adv.device)
            for i in range(0, per_member, self.minibatch):
                self.minibatch_step(obs_f, act_f, logp_f, adv_f, ret_f, perm, i, min(self.minibatch, per_member - i))
        st = self.stats_buf.tolist()   # of every member's last minibatch
        log_std = [float(x) for x in self.flat[:, (self.n_params - 1) // 2].tolist()]
        ent = [x + 0.5 * (1.0 + math.log(2.0 * math.pi)) for x in log_std]
        return {"pg": [-r[0] for r in st], "vf": [0.5 * r[1] for r in st], "entropy": ent, "clip_frac": [r[2] for r in st]}

    def iterate(self):
        """collect() + update(); per-member lists of mean_step_reward, pg, vf, entropy, clip_frac."""
        obs_b, act_b, logp_b, adv, ret, rew = self.collect()
        stats = self.update(obs_b, act_b, logp_b, adv, ret)
        stats["mean_step_reward"] = rew.reshape(rew.shape[0], self.members, self.n_member).mean(dim=(0, 2)).tolist()
        return stats

    def evolve(self, scores, frac=0.25, factors=(0.8, 1.2), explore=("lr", "ent_coef"), bounds=None, seed=0):
        """The step between two generations of population-based training, one launch (pcc_pbt_evolve, include/pcc_policy.h): the
        n_cut = int(frac * members) members with the lowest `scores` (K numbers or a tensor, larger is better, NaN last) each
        take over the parameters, Adam's moments and the hyper-parameters of a member drawn from the best n_cut, and the
        hyper-parameters named in `explore` are multiplied by one of the two `factors` and clamped to `bounds` ({name: (lo, hi)}).
        The draws are Philox's of (seed, self.generation, member): a run repeats and resumes bit for bit.  Returns (parent, rank)
        as device int32 tensors -- parent[m] == m for a member that was not replaced -- without synchronising.  The host mirror
        hyper_rows is stale from here on (None): hypers() reads the rows back."""
        from .native import lib
        if not 0.0 <= frac <= 0.5:
            raise ValueError("evolve: frac = %r (0 .. 0.5: the worst members are replaced from as many of the best)" % (frac,))
        dev = self.env.device
        score = torch.as_tensor(scores).detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        if score.numel() != self.members:
            raise ValueError("evolve: %d scores for %d members" % (score.numel(), self.members))
        ex = torch.tensor(explore_matrix(factors, explore, bounds), dtype=torch.float32, device=dev)
        parent = torch.empty(self.members, dtype=torch.int32, device=dev)
        rank = torch.empty(self.members, dtype=torch.int32, device=dev)
        rc = lib().pcc_pbt_evolve(_ptr(score), self.members, int(frac * self.members), _ptr(self.flat), _ptr(self.adam_m), _ptr(self.adam_v),
                                  self.param_stride, self.n_params, _ptr(self.hyper), _ptr(ex), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                  self.generation & 0xFFFFFFFF, _ptr(parent), _ptr(rank), self._stream())
        if rc != 0:
            raise RuntimeError("pcc_pbt_evolve failed (%d)" % rc)
        if self.normalize_obs:   # weights without their normaliser are meaningless: a replaced member takes its parent's too
            self.obs_norm.inherit(parent)
        self.generation += 1
        self.hyper_rows = None
        return parent, rank

    def hypers(self):
        """Every member's hyper row as the device holds it now ([members][8] floats, a list).  A synchronise: for logging."""
        return self.hyper.tolist()

    def state_dict(self):
        """Everything the next iterate() depends on (PPO.state_dict's contract): the flat block, Adam's state and step, hyper, the
        observation, the generator states and the env's snapshot; and the generation the next evolve() draws with."""
        dev = torch.device(self.env.device)
        sd = {"format": "population-1", "members": self.members, "obs_dim": int(self.env.obs_dim), "n_envs": int(self.env.n_envs),
              "arch": self.arch, "flat": self.flat.detach().clone(), "adam_m": self.adam_m.clone(), "adam_v": self.adam_v.clone(),
              "adam_t": int(self.adam_t), "generation": int(self.generation), "hyper": self.hyper.clone(), "obs": self.obs.detach().clone(),
              "torch_rng": torch.get_rng_state(), "device_rng": torch.cuda.get_rng_state(dev), "env": self.env.snapshot()}
        if self.normalize_obs:   # (without it the keys are what they were)
            sd.update(normalize_obs=True, obs_norm=self.obs_norm.state_dict(), raw_obs=self.raw_obs.detach().clone())
        return sd

    def load_state_dict(self, sd):
        """Continue from a state_dict() of a PopulationPPO of the same construction (env configuration, members, arch)."""
        dev = torch.device(self.env.device)
        if sd.get("format") != "population-1":
            raise ValueError("not a PopulationPPO.state_dict() of this version")
        mine = (self.members, int(self.env.obs_dim), int(self.env.n_envs), tuple(self.arch))
        theirs = (sd["members"], sd["obs_dim"], sd["n_envs"], tuple(sd["arch"]))
        if mine != theirs:
            raise ValueError("the checkpoint is of another population: (members, obs_dim, n_envs, arch) = %s; this one: %s" % (theirs, mine))
        _check_normalize(sd, self.normalize_obs)
        self.env.restore(sd["env"])
        with torch.no_grad():
            self.flat.copy_(sd["flat"])       # (the policies' parameters are views of its rows)
            self.adam_m.copy_(sd["adam_m"])
            self.adam_v.copy_(sd["adam_v"])
            self.hyper.copy_(sd["hyper"])
        self.hyper_rows = [[float(x) for x in r] for r in self.hyper.tolist()]
        self.adam_t = int(sd["adam_t"])
        self.generation = int(sd.get("generation", 0))   # (a checkpoint from before evolve() has none)
        self.obs = sd["obs"].to(dev).clone()
        if self.normalize_obs:
            self.obs_norm.load_state_dict(sd["obs_norm"])
            self.raw_obs = sd["raw_obs"].to(dev).clone()
        torch.set_rng_state(sd["torch_rng"].cpu())
        torch.cuda.set_rng_state(sd["device_rng"].cpu(), dev)
