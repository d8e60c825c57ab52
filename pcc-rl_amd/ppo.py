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

Two trainers share this module.  PPO is the single policy: a rollout is one of four strategies
(PPO._rollout_*: the policy inside the env's launches, the double-buffered loop over a GroupedNetworkEnv's groups, the fused
loop, the framework loop), the update the fused step or autograd.  PopulationPPO is K learners on slices of one env batch, one
library call per stage for all of them, and evolve() between generations.  What the two have in common is written once:
_RolloutRows (the buffers of a rollout, the observation normaliser's place in it, the fused loop, and the hand-over of the reward
and done rows to the episode ledger of track_episodes=True: DESIGN.md section 21, and to the reward normaliser of
normalize_reward=True: section 22), _Trainer (the options -- among them the update diagnostics and the KL guard of
diagnostics=True / target_kl: updiag.UpdateDiagnostics, section 23, and the limit on the gradient norm of max_grad_norm:
gradclip.GradClip, section 24 --, the first observation, the
checkpoint's common part) and native.call / native.current_stream.  They stay two classes: PPO draws its
permutations with randperm and takes the last value from the torch module, and a merge would change its numbers.

rng="philox" (both trainers) takes the rollout's noise, every epoch's minibatch order and the standardised
advantages from streams.LearnerStreams: each learner owns a 64-bit key made from its seed, and what it draws is a pure function of
(key, iteration, step or epoch, its own local sample index).  There PPO takes the last value from pcc_policy_act too, and PPO(seed=s)
on a handle of a member's envs, PopulationPPO(members=1, seeds=[s]) on it and the member with seed s of any population compute the
same bits.  The default, rng="torch", is everything above as it was.

bootstrap_time_limit=True (both trainers): every done of this env is the step limit, so the advantage
estimation bootstraps from the value of the observation an episode ended in -- rebuilt from the rollout's rows and step records
(timelimit.TimeLimitBootstrap), valued with the rollout's own parameters, read by pcc_gae_boot / pcc_gae_boot_pop.  The default,
False, is everything above as it was.

objective=... (both trainers): what the learner is trained for.  Every rollout keeps its step records, and when
it ends its reward rows are recomputed from them under the learner's weights (objective.RewardObjective, one library call for all
members): the ledger, the reward normaliser, the advantage estimation and what collect() returns see those rows; the env's own stay
in self.env_rew_b.  The default, None, is everything above as it was.
"""
import math

import torch
from torch import nn

from .env import BatchedNetworkEnv, _ptr
from .native import call, current_stream, lib
from .episodes import EpisodeLedger
from .gradclip import GradClip, limits as _grad_limits
from .objective import RewardObjective
from .obsnorm import ObsNormalizer
from .rewnorm import RewardNormalizer
from .streams import LearnerStreams
from .timelimit import TimeLimitBootstrap
from .updiag import UpdateDiagnostics


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
                                  _ptr(noise if stochastic else None), None, _ptr(a), _ptr(logp), _ptr(v), current_stream(obs.device))
        if rc != 0:   # a shape outside the library's domain (include/pcc_policy.h: pcc_ppo_supported)
            _warn_once("pcc_policy_act has no kernel for %d observations x hidden %d-%d: the policy forward runs on the framework "
                       "path (several times slower)" % (D, h1, h2))
            a2, logp2, v2 = self.act(obs, stochastic)
            if out is not None:
                a.copy_(a2.reshape(-1)); logp.copy_(logp2); v.copy_(v2)
            return a2, logp2, v2
        return a.reshape(n, 1), logp, v


def gae(rewards, values, dones, last_value, gamma=0.99, lam=0.95, term_value=None, term_count=None):
    """Generalised advantage estimation over [T, N] tensors.  dones[t] marks that the env was reset
    after step t (the next observation belongs to a new episode).
    term_value [n_slots, N] with term_count [N] (timelimit.terminal_observations: every env's number of dones in these rows):
    time-limit bootstrapping, the restatement of pcc_gae_boot -- at a done the next value is term_value[slot] of that env, slot =
    its dones in the rows before t (0 for a slot >= n_slots), and the running sum restarts at delta; the other rows are what they
    are without it."""
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    running = torch.zeros_like(last_value)
    next_value = last_value
    if term_value is not None:
        if term_count is None:
            raise ValueError("gae: term_value needs term_count")
        n_slots = term_value.shape[0]
        slot = term_count.to(torch.int64).clone()
    for t in range(T - 1, -1, -1):
        alive = 1.0 - dones[t].to(rewards.dtype)
        delta = rewards[t] + gamma * next_value * alive - values[t]
        running = delta + gamma * lam * alive * running
        if term_value is not None:
            d = dones[t].to(torch.bool)
            slot = slot - d.to(torch.int64)
            stored = d & (slot >= 0) & (slot < n_slots)
            v_term = term_value.gather(0, slot.clamp(0, n_slots - 1).unsqueeze(0))[0]
            v_term = torch.where(stored, v_term, torch.zeros_like(v_term))
            running = torch.where(d, rewards[t] + gamma * v_term - values[t], running)
        adv[t] = running
        next_value = values[t]
    return adv, adv + values


def gae_fused(rewards, values, dones, last_value, gamma=0.99, lam=0.95):
    """gae() as one launch of the HIP library (pcc_gae: thread = env, T steps backwards) for fp32 [T, N] rows on the GPU."""
    if not (rewards.is_cuda and rewards.dtype == torch.float32 and rewards.dim() == 2):
        return gae(rewards, values, dones, last_value, gamma, lam)
    T, N = rewards.shape
    rewards, values, last_value = rewards.contiguous(), values.contiguous(), last_value.contiguous().float()
    d8 = dones.contiguous().view(torch.uint8) if dones.dtype == torch.bool else dones.to(torch.uint8).contiguous()
    adv, ret = torch.empty_like(rewards), torch.empty_like(rewards)
    call("pcc_gae", _ptr(rewards), _ptr(values), _ptr(d8), _ptr(last_value), T, N, gamma, lam, _ptr(adv), _ptr(ret),
         current_stream(rewards.device))
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


class _RolloutRows(object):
    """The rows of one rollout of T steps of N envs, for both trainers: obs[T + 1] (row t: what the policy saw at step t; row T:
    the last), act, logp, val, rew, done.  `dst` is what the env writes its observations into, row t + 1 for step t: obs itself,
    or, with an observation normaliser, raw rows of its own -- after each step ONE normalise launch then fills the row the policy
    reads.  The statistics are frozen during the rollout (logp_old, the values and the update all see the same inputs) and
    updated once at its end."""

    def __init__(self, agent, T, N):
        dev, D = agent.env.device, agent.env.obs_dim
        self.T, self.N = T, N
        self.obs = torch.empty((T + 1, N, D), device=dev)
        self.act = torch.empty((T, N, 1), device=dev)
        self.logp, self.val, self.rew = (torch.empty((T, N), device=dev) for _ in range(3))
        self.done = torch.empty((T, N), dtype=torch.bool, device=dev)
        # with bootstrap_time_limit every step's float64 record: what the terminal observations are rebuilt from (section 26); with
        # an objective: what the learner's reward rows are computed from (section 27).  One buffer for both.
        keep = agent.bootstrap_time_limit or agent.objective is not None
        self.steps = torch.empty((T, N, 19), dtype=torch.float64, device=dev) if keep else None
        self.norm = agent.obs_norm if agent.normalize_obs else None
        if self.norm is None:
            self.dst = self.obs
            self.obs[0] = agent.obs
        else:
            self.dst = torch.empty((T + 1, N, D), device=dev)
            self.dst[0] = agent.raw_obs
            self.norm.normalise(self.dst[0], self.obs[0])

    def stepped(self, t):
        """After the env wrote row t + 1 of dst."""
        if self.norm is not None:
            self.norm.normalise(self.dst[t + 1], self.obs[t + 1])

    def run(self, env, noise, act):
        """The fused loop: per step act(observation row, noise row, action, log-probability and value rows) -- one policy launch --
        and the env's step from that action row into the next rows: tensors in, tensors out, no framework launch, no copy."""
        for t in range(self.T):
            act(self.obs[t], noise[t], self.act[t].reshape(self.N), self.logp[t], self.val[t])
            env.step_into(self.act[t], self.dst[t + 1], self.rew[t], self.done[t], steps_out=self.step_row(t))
            self.stepped(t)

    def step_row(self, t, lo=None, hi=None):
        """Row t of the step records (of the envs lo .. hi - 1), or None when the rollout keeps none."""
        return None if self.steps is None else self.steps[t] if lo is None else self.steps[t, lo:hi]

    def finish(self, agent):
        """The agent's observation for the next rollout, the normaliser's update from rows 0 .. T - 1 (what the policy saw) and,
        with track_episodes, the reward and done rows into the episode ledger (one library call, whichever way the rows were
        filled); returns the last observation row.  With normalize_reward the raw reward and done rows then update the reward
        normaliser, and the same rows, scaled with the updated statistics (as VecNormalize does: the first rollout is not divided
        by nothing), are what the advantage estimation reads: self.rew_gae, kept as agent.rew_norm_b.  self.rew stays raw.
        With bootstrap_time_limit the terminal observations are rebuilt here from the raw rows and, with an observation normaliser,
        normalised BEFORE its update: with the statistics every other row of this rollout was normalised with.
        With an objective, FIRST of all, the rows the env wrote become agent.env_rew_b and self.rew the objective's rows of the step
        records: everything below, and whoever reads self.rew after this call, sees the learner's reward.  The ledger then has the
        step-record channel "reward" beside channel 0: the env's own returns."""
        T = self.T
        agent.obs = self.obs[T].clone()
        if agent.objective is not None:
            agent.env_rew_b, agent.steps_b = self.rew, self.steps
            self.rew = agent.objective.apply(self.steps)
        if agent.track_episodes:
            agent._episodes_before = agent.ledger.totals()[:, :3].clone()
            agent.ledger.update(self.rew, self.done, self.steps)   # (the records are read by a ledger with step-record channels only)
        self.rew_gae = self.rew
        if agent.normalize_reward:
            agent.rew_norm.update(self.rew, self.done, agent._reward_gamma())
            self.rew_gae = agent.rew_norm_b = agent.rew_norm.normalise(self.rew)
        if agent.bootstrap_time_limit:
            agent.time_limit.terminal(self.dst, self.steps, self.done, self.norm)
            agent.steps_b = self.steps
        if self.norm is not None:
            agent.raw_b, agent.raw_obs = self.dst, self.dst[T].clone()
            self.norm.update(self.dst[:T])
        return self.obs[T]


class _Trainer(object):
    """What PPO and PopulationPPO do alike outside a rollout: the normalize_obs option, the first observation, and the part of
    a checkpoint that does not depend on how the parameters are kept."""

    bootstrap_time_limit, time_limit, steps_b = False, None, None   # (off until _set_time_limit says otherwise)
    objective, env_rew_b = None, None                                # (off until _set_objective says otherwise)

    def _set_normalize(self, env, normalize_obs, policy_in_step=False):
        """normalize_obs needs the rows between the env and the policy: not with the policy inside the env's launches."""
        self.normalize_obs = bool(normalize_obs)
        if not self.normalize_obs:
            return
        if policy_in_step:
            raise ValueError("normalize_obs=True cannot be combined with policy_in_step=True: the policy inside the env's launches "
                             "(pcc_rollout) reads the raw observation rows, not the normalised ones")
        if hasattr(env, "groups"):
            raise ValueError("normalize_obs=True is not supported over a GroupedNetworkEnv: its groups are stepped on their own streams "
                             "and the policy reads the raw observation rows there")

    def _set_rng(self, env, rng, arch=None, fused_update=True):
        """rng: "torch" -- the rollout's noise and the minibatch permutations from torch's global device generator, the advantages
        standardised with torch reductions -- or "philox": all three from streams.LearnerStreams, made once the
        env's device is known (_make_streams).  self.iteration counts the collect() calls under "philox": the counter of the draws.
        arch=None (PopulationPPO): the caller's own refusals already leave the fused paths alone."""
        who = type(self).__name__
        if rng not in ("torch", "philox"):
            raise ValueError('%s: rng = %r ("torch" or "philox")' % (who, rng))
        self.rng, self.streams, self.iteration, self._perm_buf = rng, None, 0, None
        if rng == "torch" or arch is None:
            return
        if torch.device(env.device).type != "cuda" or env.n_senders != 1 or len(arch) != 2:
            raise ValueError('%s(rng="philox") needs the fused rollout (a two-hidden-layer policy, one sender, on the GPU): the framework '
                             "rollout draws its actions from torch's generator" % who)
        if not fused_update:
            raise ValueError('%s(rng="philox") needs the fused update (fused_update=True): the framework update draws its permutations '
                             "from torch's generator" % who)

    def _make_streams(self, seeds):
        if self.rng == "philox":
            self.streams = LearnerStreams(seeds, int(self.env.n_envs), self.env.device)

    def _order(self, T, epoch):
        """The minibatch order of this iteration's epoch `epoch` under rng="philox": [members][T * n_m] global sample indices, in a
        buffer that the next call overwrites (the launches that read it are ahead of that one on the stream)."""
        n = T * self.streams.n_member
        if self._perm_buf is None or self._perm_buf.shape[1] != n:
            self._perm_buf = torch.empty((self.streams.members, n), dtype=torch.int64, device=self.env.device)
        return self.streams.order(T, self.iteration, epoch, out=self._perm_buf)

    def _set_reward_norm(self, env, normalize_reward, clip_reward, norm_eps, members=1):
        """normalize_reward: a rewnorm.RewardNormalizer over the env batch, fed by every rollout after it ended (DESIGN.md section
        22): it works with every rollout path."""
        self.normalize_reward, self.rew_norm, self.rew_norm_b = bool(normalize_reward), None, None
        if not self.normalize_reward:
            return
        if torch.device(env.device).type != "cuda":
            raise ValueError("normalize_reward=True runs HIP kernels: it needs the env on the GPU (device=%r); there is no CPU path"
                             % (env.device,))
        if env.n_senders != 1:
            raise ValueError("normalize_reward=True needs one sender per env (n_senders = %d): the normaliser's rows are [T][n_envs]" % env.n_senders)
        self.rew_norm = RewardNormalizer(int(env.n_envs), members, clip_reward, norm_eps, device=env.device)

    def _set_time_limit(self, env, bootstrap_time_limit, horizon, members=1):
        """bootstrap_time_limit: a timelimit.TimeLimitBootstrap over the env batch: every rollout keeps its
        step records, its terminal observations are rebuilt when it ends, and the advantage estimation bootstraps from their values
        under the rollout's own parameters.  It works with every rollout path; it holds nothing between two rollouts."""
        self.bootstrap_time_limit, self.time_limit, self.steps_b = bool(bootstrap_time_limit), None, None
        if self.bootstrap_time_limit:
            self.time_limit = TimeLimitBootstrap(env, horizon, members)   # (raises ValueError off the GPU or with two senders)

    def _set_objective(self, env, objective, members=1):
        """objective: an objective.RewardObjective over the env batch, or what makes one: a dict of term
        weights, a sequence of them, or one of either per member.  Every rollout keeps its step records and its reward rows are the
        objective's; it works with every rollout path.  Call it before _set_episodes: the ledger then carries the env's own reward
        as a step-record channel."""
        self.objective, self.env_rew_b = None, None
        if objective is None:
            return
        if torch.device(env.device).type != "cuda":
            raise ValueError("objective=... runs HIP kernels: it needs the env on the GPU (device=%r); there is no CPU path" % (env.device,))
        if env.n_senders != 1:
            raise ValueError("objective=... needs one sender per env (n_senders = %d): the rows are [T][n_envs]" % env.n_senders)
        if isinstance(objective, RewardObjective):
            if (objective.n_envs, objective.members) != (int(env.n_envs), members):
                raise ValueError("objective: a RewardObjective of (n_envs, members) = (%d, %d) for a trainer of (%d, %d)"
                                 % (objective.n_envs, objective.members, env.n_envs, members))
            self.objective = objective
        else:
            self.objective = RewardObjective(int(env.n_envs), members, objective, device=env.device)

    def _set_diagnostics(self, env, diagnostics, target_kl, diag_rows, horizon, members=1):
        """diagnostics / target_kl: an updiag.UpdateDiagnostics over the env batch, run after every epoch of update() (DESIGN.md
        section 23).  target_kl implies diagnostics; diag_rows=R reads about R of the horizon's rows (every max(1, T // R)-th)."""
        self.target_kl = None if target_kl is None else float(target_kl)
        self.diagnostics, self.diag = bool(diagnostics) or target_kl is not None, None
        if not self.diagnostics:
            return
        if self.target_kl is not None and not self.target_kl > 0.0:
            raise ValueError("target_kl = %r (> 0, or None for no guard)" % (target_kl,))
        if diag_rows is not None and int(diag_rows) < 1:
            raise ValueError("diag_rows = %r (>= 1, or None for every row)" % (diag_rows,))
        if torch.device(env.device).type != "cuda":
            raise ValueError("diagnostics=True / target_kl run HIP kernels: they need the env on the GPU (device=%r); there is no CPU path"
                             % (env.device,))
        if env.n_senders != 1:
            raise ValueError("diagnostics=True / target_kl need one sender per env (n_senders = %d): the rows are [T][n_envs]" % env.n_senders)
        row_step = 1 if diag_rows is None else max(1, int(horizon) // int(diag_rows))
        self.diag = UpdateDiagnostics(int(env.n_envs), members, env.device, row_step)

    def _set_grad_clip(self, env, max_grad_norm, fused_update=True, members=1):
        """max_grad_norm: every optimiser step goes through pcc_ppo_minibatch_step_clip_pop with the members'
        limits in column 5 of hyper; None: the steps are the unclipped entry points', as before.  The buffers (gradclip.GradClip)
        are made once the parameter blocks are."""
        who = type(self).__name__
        self.max_grad_norm, self.grad_clip = None, None
        if max_grad_norm is None:
            return
        self.max_grad_norm = _grad_limits(max_grad_norm, members, who)
        if not fused_update:
            raise ValueError("%s(max_grad_norm=...) needs the fused update (fused_update=True): the clipped step is a HIP kernel beside "
                             "the fused step" % who)
        if torch.device(env.device).type != "cuda":
            raise ValueError("max_grad_norm runs HIP kernels: it needs the env on the GPU (device=%r); there is no CPU path" % (env.device,))

    def _kl_limit(self):
        """What pcc_update_diag_pop stops a member at: 1.5 x the target, as stable-baselines3 and Spinning Up do; 0: no guard."""
        return 0.0 if self.target_kl is None else 1.5 * self.target_kl

    def _set_episodes(self, env, track_episodes, members=1):
        """track_episodes: an episodes.EpisodeLedger over the env batch, fed by every rollout."""
        self.track_episodes, self.ledger = bool(track_episodes), None
        if not self.track_episodes:
            return
        if env.n_senders != 1:
            raise ValueError("track_episodes=True needs one sender per env (n_senders = %d): the ledger's rows are [T][n_envs]" % env.n_senders)
        # under an objective channel 0 is the learner's reward; the env's own stays beside it as the step-record channel "reward"
        self.ledger = EpisodeLedger(int(env.n_envs), members, ("reward",) if self.objective is not None else (), device=env.device)

    def _episode_stats(self):
        """The episodes finished in the last rollout, as the difference of the ledger's totals after and before it: per member
        (episodes, mean return, mean length), NaN without a finished episode.  A synchronise."""
        nan = float("nan")
        rows = (self.ledger.totals()[:, :3] - self._episodes_before).tolist()
        return ([int(r[0]) for r in rows], [r[2] / r[0] if r[0] > 0 else nan for r in rows],
                [r[1] / r[0] if r[0] > 0 else nan for r in rows])

    def _first_obs(self, members, clip_obs, norm_eps):
        """Reset the env; with normalize_obs every member gets its own moments of its own columns (obsnorm.ObsNormalizer)."""
        self.obs = self.env.reset().clone()
        if self.normalize_obs:
            self.obs_norm = ObsNormalizer(self.env.obs_dim, members, clip_obs, norm_eps, device=self.env.device)
            self.raw_obs = self.obs
            self.obs = self.obs_norm.normalise(self.raw_obs)

    def _adam_state(self):
        return dict(flat=self.flat.detach().clone(), adam_m=self.adam_m.clone(), adam_v=self.adam_v.clone(), adam_t=int(self.adam_t))

    def _load_adam_state(self, sd):
        with torch.no_grad():
            self.flat.copy_(sd["flat"])   # (the modules' parameters are views of it: share_flat)
            self.adam_m.copy_(sd["adam_m"])
            self.adam_v.copy_(sd["adam_v"])
        self.adam_t = int(sd["adam_t"])

    def _common_state(self):
        """The keys both state_dict()s end with: the observation the next rollout starts from, torch's CPU and device generator
        states (the rollout's noise and the minibatch permutations come from the device's), the env's snapshot, and with
        normalize_obs the normaliser and the raw observation, with track_episodes the episode ledger, with normalize_reward the
        reward normaliser (without an option the keys are what they were before it)."""
        dev = torch.device(self.env.device)
        sd = {"obs": self.obs.detach().clone(), "torch_rng": torch.get_rng_state(),
              "device_rng": torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None, "env": self.env.snapshot()}
        if self.normalize_obs:
            sd.update(normalize_obs=True, obs_norm=self.obs_norm.state_dict(), raw_obs=self.raw_obs.detach().clone())
        if self.track_episodes:
            sd.update(track_episodes=True, episodes=self.ledger.state_dict())
        if self.normalize_reward:
            sd.update(normalize_reward=True, rew_norm=self.rew_norm.state_dict())
        if self.bootstrap_time_limit:   # (the option only: it holds nothing between two rollouts)
            sd.update(bootstrap_time_limit=True)
        if self.objective is not None:   # the weights: what the value network's targets are made of
            sd.update(objective=True, objective_state=self.objective.state_dict())
        if self.diagnostics:   # (the options only: the buffers live for one update)
            sd.update(diagnostics=True, target_kl=self.target_kl, diag_row_step=self.diag.row_step)
        if self.rng == "philox":   # the learners' keys and the counter of their draws (the generator states above are not read)
            sd.update(rng="philox", streams=self.streams.state_dict(), iteration=int(self.iteration))
        return sd

    def _restore(self, sd):
        """What both load_state_dict()s do after their own checks: the env from its snapshot (it must have been reset once: the
        constructor did that), the parameters and the optimiser (self._load_params), the observation, the generator states."""
        dev = torch.device(self.env.device)
        theirs = bool(sd.get("normalize_obs", False))
        if theirs != self.normalize_obs:
            raise ValueError("the checkpoint was written with normalize_obs=%s, this object has normalize_obs=%s: weights without "
                             "their normaliser are meaningless" % (theirs, self.normalize_obs))
        theirs = bool(sd.get("track_episodes", False))
        if theirs != self.track_episodes:
            raise ValueError("the checkpoint was written with track_episodes=%s, this object has track_episodes=%s: the running "
                             "episodes of the env's snapshot and the ledger belong together" % (theirs, self.track_episodes))
        theirs = bool(sd.get("normalize_reward", False))
        if theirs != self.normalize_reward:
            raise ValueError("the checkpoint was written with normalize_reward=%s, this object has normalize_reward=%s: a value "
                             "network without the scale of its targets is meaningless" % (theirs, self.normalize_reward))
        theirs = bool(sd.get("bootstrap_time_limit", False))
        if theirs != self.bootstrap_time_limit:
            raise ValueError("the checkpoint was written with bootstrap_time_limit=%s, this object has bootstrap_time_limit=%s: the "
                             "value network was trained towards other targets" % (theirs, self.bootstrap_time_limit))
        theirs = bool(sd.get("objective", False))
        if theirs != (self.objective is not None):
            raise ValueError("the checkpoint was written with objective=%s, this object has objective=%s: the value network was "
                             "trained towards another reward" % ("..." if theirs else None, "..." if self.objective is not None else None))
        theirs = (bool(sd.get("diagnostics", False)), sd.get("target_kl"), sd.get("diag_row_step"))
        mine = (self.diagnostics, self.target_kl, self.diag.row_step if self.diagnostics else None)
        if theirs != mine:
            raise ValueError("the checkpoint was written with (diagnostics, target_kl, row step) = %s, this object has %s: the KL guard "
                             "decides which updates are applied" % (theirs, mine))
        theirs = sd.get("rng", "torch")
        if theirs != self.rng:
            raise ValueError("the checkpoint was written with rng=%r, this object has rng=%r: the two modes draw different rollouts and "
                             "minibatches" % (theirs, self.rng))
        self.env.restore(sd["env"])
        self._load_params(sd)
        if self.rng == "philox":
            self.streams.load_state_dict(sd["streams"])
            self.iteration = int(sd["iteration"])
        if self.normalize_reward:
            self.rew_norm.load_state_dict(sd["rew_norm"])
        if self.objective is not None:
            self.objective.load_state_dict(sd["objective_state"])
        if self.track_episodes:
            self.ledger.load_state_dict(sd["episodes"])
        self.obs = sd["obs"].to(dev).clone()
        if self.normalize_obs:
            self.obs_norm.load_state_dict(sd["obs_norm"])
            self.raw_obs = sd["raw_obs"].to(dev).clone()
        torch.set_rng_state(sd["torch_rng"].cpu())
        if dev.type == "cuda" and sd.get("device_rng") is not None:
            torch.cuda.set_rng_state(sd["device_rng"].cpu(), dev)


class PPO(_Trainer):
    def __init__(self, env, arch=(32, 16), gamma=0.99, lam=0.95, clip=0.2, ent_coef=0.01, lr=1e-3,
                 epochs=4, minibatch=None, horizon=64, seed=0, fused_update=True, policy_in_step=False,
                 normalize_obs=False, clip_obs=10.0, norm_eps=1e-8, track_episodes=False, normalize_reward=False, clip_reward=10.0,
                 diagnostics=False, target_kl=None, diag_rows=None, max_grad_norm=None, rng="torch",
                 bootstrap_time_limit=False, objective=None):
        """minibatch None = a quarter of the rollout, at least 2048: the reference's ratio (optim_batchsize 2048 of a
        timesteps_per_actorbatch of 8192, stable_solve.py:52) -- at 65 536 envs x 64 steps a fixed 2048 would be 2 048
        optimiser steps per epoch, thousands of launches of a few microseconds of work each.
        policy_in_step: collect() runs the horizon as ONE closed-loop library call per env (group) -- env.rollout, pcc_rollout:
        the policy inside the env's own launches -- with the same numbers, bit for bit, as the policy kernel + step_into loop.
        normalize_obs: the policy sees clamp((obs - mean) / sqrt(var + norm_eps), -clip_obs, clip_obs) with the running moments of
        the raw rows (obsnorm.ObsNormalizer): frozen during a rollout, updated once at its end.
        track_episodes: every rollout's reward and done rows go into an episode ledger (episodes.EpisodeLedger, self.ledger) and
        iterate() adds episodes, mean_episode_return and mean_episode_length of the episodes that rollout finished.
        normalize_reward: the advantage estimation reads clamp(reward / sqrt(var + norm_eps), -clip_reward, clip_reward), var the
        running variance of every env's discounted return (rewnorm.RewardNormalizer, self.rew_norm), updated
        at the end of a rollout and applied to that rollout's rows (self.rew_norm_b).  What collect() returns and iterate() reports
        stays raw.
        diagnostics: after every epoch of update() the approximate KL divergence between the rollout's policy and the updated one, the
        clip fraction over the whole rollout and the explained variance of the value function are computed on the device
        (updiag.UpdateDiagnostics, self.diag), and update() adds approx_kl, clip_fraction, explained_variance,
        max_log_ratio, nonfinite and epochs_run from the check after the last epoch.  The parameters are what they are without it.
        target_kl (implies diagnostics): once the approximate KL exceeds 1.5 x target_kl after an epoch -- or is NaN -- the later
        minibatches of this update are gradient-only (the parameters and Adam's moments stay; Adam's step count goes on), decided on
        the device without a synchronise.  diag_rows=R: the checks read every max(1, horizon // R)-th row.  Both need the fused
        update.
        max_grad_norm=M (>= 0): every optimiser step limits the global norm of its gradient to M, as torch.nn.utils.clip_grad_norm_
        does, and a step whose gradient is not finite changes neither the parameters nor Adam's moments (Adam's step count goes on);
        M = 0 is that guard alone.  One library call per step beside the fused step's kernels (gradclip.GradClip, self.grad_clip;
        DESIGN.md section 24); update() adds grad_norm (the last step's), max_grad_norm_seen, clipped_steps and skipped_steps.  A
        step that neither clips nor skips leaves the bits the unclipped step leaves.  Needs the fused update.
        rng="philox": the rollout's noise, every epoch's minibatch order and the standardised advantages come from the learner's own
        keyed streams on the device (streams.LearnerStreams, self.streams) -- functions of (the key made from
        `seed`, self.iteration, step or epoch, sample index), none of torch's generators -- and the last value of a rollout from
        pcc_policy_act: the run equals PopulationPPO(members=1, seeds=[seed], rng="philox") and the member with this seed of any
        population on the same env ids, bit for bit.  Needs the fused rollout and the fused update; works with every other option.
        The default "torch" draws from torch's global device generator, as before.
        bootstrap_time_limit: every done of this env is a truncation at max_steps, never a terminal state: the advantage estimation
        bootstraps from the value of the observation the episode ended in instead of from zero (timelimit.TimeLimitBootstrap,
        self.time_limit).  The env overwrites that observation with the next episode's first one, so it is
        rebuilt, bit for bit, from the rollout's observation rows and step records (pcc_terminal_obs; the records are 152 bytes per
        sample, held while the option is on), valued with the rollout's own parameters and read by pcc_gae_boot.  A rollout without
        a done leaves the bits it leaves without the option.  The rewards collect() returns, the ledger, the reward normaliser and
        evolve()'s scores are untouched.  One sender per env; works with every rollout path and every other option.
        objective: what the controller is trained for, as weights over the step records' metrics (objective.RewardObjective,
        self.objective): a dict such as {"throughput": 10, "latency": -1e3, "loss": -2e3} -- that one is
        RewardObjective.DEFAULT, the env's own reward, which reproduces it bit for bit --, six numbers in the order of
        objective.TERMS, or a RewardObjective.  The rollout keeps its step records (152 bytes per sample, the buffer
        bootstrap_time_limit holds) and its reward rows are recomputed from them when it ends: the episode ledger's channel 0, the
        reward normaliser, the advantage estimation, collect()'s sixth value and mean_step_reward are the objective's; the env's own
        rows stay in self.env_rew_b, its returns in the ledger's channel "reward" and in the env's last_return.  iterate() adds
        objective_terms: {term: mean weighted term}.  One sender per env; works with every rollout path and every other option."""
        self._set_rng(env, rng, arch, fused_update)
        self._set_time_limit(env, bootstrap_time_limit, horizon)
        self._set_objective(env, objective)
        self._set_grad_clip(env, max_grad_norm, fused_update)
        if self.max_grad_norm is not None:
            self.max_grad_norm = self.max_grad_norm[0]   # (one policy: a number, read at every update like lr: _hyper_now)
        if (diagnostics or target_kl is not None) and not fused_update:
            raise ValueError("PPO(diagnostics=True / target_kl) needs the fused update (fused_update=True): the framework path has no "
                             "diagnostics")
        self._set_diagnostics(env, diagnostics, target_kl, diag_rows, horizon)
        if policy_in_step and torch.device(env.device).type != "cuda":
            raise ValueError("PPO(policy_in_step=True) runs the policy inside the env's HIP launches: it needs the env on the GPU "
                             "(device=%r)" % (env.device,))
        self.policy_in_step = bool(policy_in_step)
        self._set_normalize(env, normalize_obs, policy_in_step)
        self._set_episodes(env, track_episodes)
        self._set_reward_norm(env, normalize_reward, clip_reward, norm_eps)
        self.env, self.gamma, self.lam, self.clip, self.ent_coef = env, gamma, lam, clip, ent_coef
        self.epochs, self.minibatch, self.horizon = epochs, minibatch, horizon
        torch.manual_seed(seed)
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
        if self.rng == "philox" and not self.fused_update:
            raise ValueError('PPO(rng="philox") needs the fused update: the library has no pcc_ppo_minibatch_step for observation length '
                             "%d, hidden %s" % (env.obs_dim, list(arch)))
        if self.fused_update:
            self.flat = self.policy.share_flat()
            self.adam_m, self.adam_v, self.adam_t = torch.zeros_like(self.flat), torch.zeros_like(self.flat), 0
            self.scratch = torch.empty(lib().pcc_ppo_scratch_floats(env.obs_dim, arch[0], arch[1]), device=env.device)
            self.stats_buf = torch.zeros(4, device=env.device)
        elif self.diagnostics or self.max_grad_norm is not None:
            raise ValueError("PPO(diagnostics=True / target_kl / max_grad_norm) needs the fused update: the library has no "
                             "pcc_ppo_minibatch_step for observation length %d, hidden %s" % (env.obs_dim, list(arch)))
        if self.diagnostics or self.max_grad_norm is not None:
            # the [1][8] hyper block the checks read the clip range from, the step of target_kl its lr, the clipped step its limit
            self.hyper = torch.zeros((1, HYPER_COLS), dtype=torch.float32, device=env.device)   # (filled at every update: _hyper_now)
            self.param_stride = (self.flat.numel() + 63) // 64 * 64   # (one member: the padding is never read or written)
        if self.max_grad_norm is not None:
            self.grad_clip = GradClip(self.param_stride, 1, env.device)
        self.opt = torch.optim.Adam(self.policy.parameters(), lr=lr, eps=self.adam_eps)
        self._first_obs(1, clip_obs, norm_eps)
        self._make_streams([seed])
        if self.minibatch is None:
            self.minibatch = max(2048, env.n_envs * horizon // 4)

    def _fused_update_ok(self):
        env = self.env
        hidden = self.policy.hidden
        if not (torch.device(env.device).type == "cuda" and hidden is not None and env.n_senders == 1):
            return False
        return lib().pcc_ppo_supported(int(env.obs_dim), hidden[0], hidden[1]) == 1

    def collect(self):
        """One rollout of `horizon` steps of every env.  The policy kernel reads the observation row the env wrote and
        writes action / log-probability / value into the rollout rows; the env reads that action row and writes the next
        observation, reward and done rows: two library calls and three kernels per step, no framework launch, no copy."""
        env, T, N = self.env, self.horizon, self.env.n_envs
        philox = self.rng == "philox"
        if philox:
            self.iteration += 1
        rows = _RolloutRows(self, T, N)
        fused = self.policy.fused_ok(rows.obs[0]) and env.n_senders == 1
        if self.policy_in_step and not fused:
            raise ValueError("PPO(policy_in_step=True) needs the fused rollout: a two-hidden-layer policy, one sender, on the GPU")
        if philox and not fused:
            raise ValueError('PPO(rng="philox") needs the fused rollout: a two-hidden-layer policy, one sender, on the GPU')
        if not fused:
            self._rollout_framework(rows)
        else:
            params = self.policy.flat_params()                     # once per rollout, not per step (a 13-tensor torch.cat)
            # the horizon's draws in one launch: torch's generator, or the learner's keyed stream of this iteration
            noise = self.streams.noise(T, self.iteration) if philox else torch.randn((T, N), device=env.device)
            if self.policy_in_step:
                self._rollout_in_step(rows, params, noise)
            elif hasattr(env, "groups"):
                self._rollout_double_buffered(rows, params, noise)
            else:
                rows.run(env, noise, lambda o, z, a, logp, v: self.policy.act_fused(o, True, params, z, (a, logp, v)))
        obs = rows.finish(self)
        if philox:   # the value output of the kernel the rollout ran, as the population takes it
            _, _, last_v = self.policy.act_fused(obs, False, params)
        else:
            with torch.no_grad():
                last_v = self.policy.value(obs)
        # never train on corrupted rollouts: an overflowed in-flight ring / an empty ring pool (a trained
        # policy can push many deep-queue envs to MAX_RATE: BatchedNetworkEnv(ring_pools=...)) is flagged, not silent
        env.check_flags()
        if self.bootstrap_time_limit:
            adv, ret = self._gae_time_limit(rows, last_v, params if fused else None)
        else:
            adv, ret = (gae_fused if fused else gae)(rows.rew_gae, rows.val, rows.done, last_v, self.gamma, self.lam)
        self.val_b, self.done_b = rows.val, rows.done
        return rows.obs[:T], rows.act, rows.logp, adv, ret, rows.rew

    def _reward_gamma(self):
        return self.gamma

    def _gae_time_limit(self, rows, last_v, params):
        """The advantage estimation under bootstrap_time_limit: the values of the terminal rows (rows.finish made them) with the
        rollout's parameters -- params: the block the fused rollout ran with, one pcc_policy_act per slot; None: the framework
        rollout, the torch module -- then pcc_gae_boot, or on the framework path its restatement gae(term_value=...)."""
        tl = self.time_limit
        if params is not None:
            tl.values(lambda o, v: self._value_fused(o, v, params))
            return tl.gae(rows.rew_gae, rows.val, rows.done, last_v, self.gamma, self.lam)
        with torch.no_grad():
            tl.values(lambda o, v: v.copy_(self.policy.value(o)))
        return gae(rows.rew_gae, rows.val, rows.done, last_v, self.gamma, self.lam, tl.term_val, tl.term_count)

    def _value_fused(self, obs, out, params):
        """out[N] = the value output of pcc_policy_act on obs [N, D] (no noise, no other output): one launch."""
        h1, h2 = self.policy.hidden
        rc = lib().pcc_policy_act(_ptr(obs), obs.shape[0], obs.shape[1], _ptr(params), h1, h2, None, None, None, None, _ptr(out),
                                  current_stream(obs.device))
        if rc != 0:   # (as act_fused: a shape outside the library's domain -- the rollout ran on the framework path too)
            _warn_once("pcc_policy_act has no kernel for %d observations x hidden %d-%d: the terminal values come from the framework "
                       "path" % (obs.shape[1], h1, h2))
            with torch.no_grad():
                out.copy_(self.policy.value(obs))

    def _rollout_in_step(self, rows, params, noise):
        """The whole horizon as one pcc_rollout per env (group): the same noise, parameters and rows as the fused loop."""
        env, T, arch = self.env, rows.T, self.policy.hidden
        dev = env.device
        outs = (rows.act, rows.logp, rows.val, rows.rew, rows.done.view(torch.uint8))
        if not hasattr(env, "groups"):
            return env.rollout(params, noise, rows.obs, *outs, steps_b=rows.steps, arch=arch)
        n = env.group_size
        cur = torch.cuda.current_stream(dev)
        # (a group's rows of [T(+1), N] buffers are strided: each group fills contiguous buffers of its own on its stream)
        parts = []
        for g, eg in enumerate(env.groups):
            lo, hi = g * n, (g + 1) * n
            env.streams[g].wait_stream(cur)
            with torch.cuda.stream(env.streams[g]):
                ob = torch.empty((T + 1, n, env.obs_dim), device=dev)
                ob[0] = rows.obs[0, lo:hi]
                bufs = (torch.empty((T, n, 1), device=dev), torch.empty((T, n), device=dev), torch.empty((T, n), device=dev),
                        torch.empty((T, n), device=dev), torch.empty((T, n), dtype=torch.uint8, device=dev))
                if rows.steps is not None:
                    bufs += (torch.empty((T, n, 19), dtype=torch.float64, device=dev),)
                eg.rollout(params, noise[:, lo:hi].contiguous(), ob, *bufs, arch=arch)   # (steps_b follows done_b)
                parts.append((lo, hi, ob, bufs))
        if rows.steps is not None:
            outs += (rows.steps,)
        for g, (lo, hi, ob, bufs) in enumerate(parts):
            cur.wait_stream(env.streams[g])
            rows.obs[1:, lo:hi] = ob[1:]
            for dst, src in zip(outs, bufs):
                dst[:, lo:hi] = src
            for tns in (ob,) + bufs:
                tns.record_stream(cur)

    def _rollout_double_buffered(self, rows, params, noise):
        """Double-buffered sampling (GroupedNetworkEnv: the same envs as G groups on their own streams): group g's policy
        kernel and env step are queued on stream g, nothing joins the groups inside the rollout -- while one group's env launches
        run out their tails (a third of the wavefront slots busy), the other group's policy kernel and
        launches fill the machine.  Same numbers as one batch: a group holds the global env ids g * n .. and reads its own
        rows of every buffer."""
        env, n = self.env, self.env.group_size
        cur = torch.cuda.current_stream(env.device)
        for s in env.streams:
            s.wait_stream(cur)                                 # the buffers and the noise were made on this stream
        for t in range(rows.T):
            for g, eg in enumerate(env.groups):
                lo, hi = g * n, (g + 1) * n
                with torch.cuda.stream(env.streams[g]):
                    self.policy.act_fused(rows.obs[t, lo:hi], True, params, noise[t, lo:hi],
                                          (rows.act[t, lo:hi].reshape(n), rows.logp[t, lo:hi], rows.val[t, lo:hi]))
                    eg.step_into(rows.act[t, lo:hi], rows.obs[t + 1, lo:hi], rows.rew[t, lo:hi], rows.done[t, lo:hi],
                                 steps_out=rows.step_row(t, lo, hi))
        for s in env.streams:
            cur.wait_stream(s)

    def _rollout_framework(self, rows):
        """The policy as a torch module and env.step(): for a policy or an env that pcc_policy_act does not cover."""
        for t in range(rows.T):
            a, logp, v = self.policy.act(rows.obs[t])
            rows.act[t], rows.logp[t], rows.val[t] = a, logp, v
            if rows.steps is not None:   # (the same library call as step(), into the rollout's rows: the step records with them)
                self.env.step_into(a, rows.dst[t + 1], rows.rew[t], rows.done[t], steps_out=rows.steps[t])
                rows.stepped(t)
                continue
            nobs, r, d, _ = self.env.step(a)
            rows.dst[t + 1] = nobs
            rows.stepped(t)
            rows.rew[t], rows.done[t] = r, d

    def update(self, obs_b, act_b, logp_b, adv, ret):
        n = obs_b.shape[0] * obs_b.shape[1]
        obs_f, act_f = obs_b.reshape(n, -1), act_b.reshape(n, -1)
        logp_f, adv_f, ret_f = logp_b.reshape(n), adv.reshape(n), ret.reshape(n)
        if self.rng == "philox":
            if adv.dim() != 2:
                raise ValueError('PPO(rng="philox").update needs the rollout\'s [T][N] advantage rows, as collect() returns them')
            adv_f = self.streams.standardise(adv.contiguous()).reshape(n)
        else:
            adv_f = (adv_f - adv_f.mean()) / (adv_f.std() + 1e-8)
        if self.fused_update:
            if self.diagnostics and obs_b.dim() != 3:
                raise ValueError("PPO(diagnostics=True).update needs the rollout's [T][N][D] observation rows, as collect() returns them")
            return self._update_fused(obs_f, act_f, logp_f, adv_f, ret_f, obs_b.shape[0])
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
        lr = self.lr if lr is None else lr
        if start < 0 or count < 1 or start + count > (perm.numel() if perm is not None else obs_f.shape[0]):
            raise ValueError("minibatch [%d, %d) outside the rollout" % (start, start + count))
        if lr != 0.0:
            self.adam_t += 1
        D = obs_f.shape[1]
        h1, h2 = self.policy.hidden
        call("pcc_ppo_minibatch_step", _ptr(obs_f), _ptr(act_f), _ptr(logp_f), _ptr(adv_f), _ptr(ret_f), _ptr(perm), start, count,
             D, h1, h2, _ptr(self.flat), _ptr(self.adam_m), _ptr(self.adam_v), max(self.adam_t, 1),
             lr, 0.9, 0.999, self.adam_eps, self.clip, self.ent_coef, _ptr(self.scratch),
             _ptr(grad_out), _ptr(self.stats_buf), current_stream(obs_f.device))

    def _hyper_now(self):
        """self.hyper from lr, clip, ent_coef, gamma, lam and the limit on the gradient norm as they are NOW: a caller may change them
        between updates (a schedule), and the guarded step and the checks must see what minibatch_step_fused would pass."""
        limit = 0.0 if self.max_grad_norm is None else _grad_limits(self.max_grad_norm, 1, "PPO")[0]
        row = [[self.lr, self.clip, self.ent_coef, self.gamma, self.lam, limit] + [0.0] * (HYPER_COLS - len(HYPER_NAMES))]
        self.hyper.copy_(torch.tensor(row, dtype=torch.float32))
        return self.hyper

    def _minibatch_step_guarded(self, obs_f, act_f, logp_f, adv_f, ret_f, perm, start, count):
        """minibatch_step_fused under target_kl: pcc_ppo_minibatch_step_pop with ONE member and the checks' hyper_live as its hyper
        block -- bit-identical to pcc_ppo_minibatch_step while the member is live, gradient-only once the
        kernel has stopped it."""
        if self.lr != 0.0:   # (as minibatch_step_fused: a gradient-only step is no step of Adam's)
            self.adam_t += 1
        h1, h2 = self.policy.hidden
        call("pcc_ppo_minibatch_step_pop", _ptr(obs_f), _ptr(act_f), _ptr(logp_f), _ptr(adv_f), _ptr(ret_f), _ptr(perm), perm.numel(),
             start, count, obs_f.shape[1], h1, h2, _ptr(self.flat), _ptr(self.adam_m), _ptr(self.adam_v), self.param_stride, 1,
             _ptr(self.diag.hyper_live), max(self.adam_t, 1), 0.9, 0.999, self.adam_eps, _ptr(self.scratch), None, _ptr(self.stats_buf),
             current_stream(obs_f.device))

    def _minibatch_step_clipped(self, obs_f, act_f, logp_f, adv_f, ret_f, perm, start, count):
        """The step under max_grad_norm: pcc_ppo_minibatch_step_clip_pop with ONE member -- the fused step's two launches as a
        gradient-only call, then the norm, the coefficient and Adam on the scaled gradient.  Its hyper block
        is self.hyper, or under target_kl the checks' hyper_live: a stopped member stays gradient-only."""
        if self.lr != 0.0:   # (as minibatch_step_fused: a gradient-only step is no step of Adam's)
            self.adam_t += 1
        h1, h2 = self.policy.hidden
        gc = self.grad_clip
        call("pcc_ppo_minibatch_step_clip_pop", _ptr(obs_f), _ptr(act_f), _ptr(logp_f), _ptr(adv_f), _ptr(ret_f), _ptr(perm), perm.numel(),
             start, count, obs_f.shape[1], h1, h2, _ptr(self.flat), _ptr(self.adam_m), _ptr(self.adam_v), self.param_stride, 1,
             _ptr(self.hyper if self.target_kl is None else self.diag.hyper_live), max(self.adam_t, 1), 0.9, 0.999, self.adam_eps,
             _ptr(self.scratch), _ptr(gc.grad), _ptr(self.stats_buf), _ptr(gc.hyper_grad), _ptr(gc.clip), gc.clip.stride(0),
             current_stream(obs_f.device))

    def _update_fused(self, obs_f, act_f, logp_f, adv_f, ret_f, T=None):
        n = obs_f.shape[0]
        obs_f, act_f = obs_f.contiguous(), act_f.reshape(n).contiguous()
        logp_f, adv_f, ret_f = logp_f.contiguous(), adv_f.contiguous(), ret_f.contiguous()
        step = self.minibatch_step_fused if self.target_kl is None else self._minibatch_step_guarded
        if self.diagnostics or self.grad_clip is not None:
            self._hyper_now()
        if self.grad_clip is not None:
            step = self._minibatch_step_clipped
            self.grad_clip.begin()
        if self.diagnostics:
            self.diag.begin(self.hyper)
        for e in range(self.epochs):
            perm = self._order(T, e)[0] if self.rng == "philox" else torch.randperm(n, device=obs_f.device)
            for i in range(0, n, self.minibatch):
                step(obs_f, act_f, logp_f, adv_f, ret_f, perm, i, min(self.minibatch, n - i))
            if self.diagnostics:   # what this epoch did, and whether the next one still updates
                self.diag.check(e + 1, obs_f.view(T, n // T, -1), act_f, logp_f, ret_f, self.val_b.contiguous(), self.flat,
                                self.param_stride, self.flat.numel(), self.policy.hidden, self.hyper, self._kl_limit())
        st = self.stats_buf.tolist()   # of the last minibatch, like the framework path
        ent = float(self.policy.log_std.detach().sum()) + 0.5 * (1.0 + math.log(2.0 * math.pi)) * self.policy.log_std.numel()
        out = {"pg": -st[0], "vf": 0.5 * st[1], "entropy": ent, "clip_frac": st[2]}
        if self.diagnostics:
            out.update({k: v[0] for k, v in self.diag.report(self.epochs).items()})
        if self.grad_clip is not None:
            out.update({k: v[0] for k, v in self.grad_clip.report().items()})
        return out

    def state_dict(self):
        """Everything the next iterate() depends on, for a checkpoint that resumes bit for bit: the parameters and Adam's state (the
        flat block with m, v, t on the fused path, the module's and the torch optimiser's state_dict on the framework path), the
        observation, the generator states and the env's snapshot (_Trainer._common_state; BatchedNetworkEnv.snapshot: not with the env
        options it refuses).  torch.save() takes it as it is."""
        sd = {"format": 1, "fused_update": self.fused_update, "obs_dim": int(self.env.obs_dim), "n_envs": int(self.env.n_envs)}
        if self.fused_update:
            sd.update(self._adam_state())
        else:
            sd.update(policy={k: v.detach().clone() for k, v in self.policy.state_dict().items()}, opt=self.opt.state_dict())
        sd.update(self._common_state())
        return sd

    def load_state_dict(self, sd):
        """Continue from a state_dict() of a PPO of the same construction (env configuration, arch, update path, normalize_obs):
        _Trainer._restore after the checks."""
        if sd.get("format") != 1:
            raise ValueError("not a PPO.state_dict() of this version")
        if bool(sd["fused_update"]) != self.fused_update or sd["obs_dim"] != int(self.env.obs_dim) or sd["n_envs"] != int(self.env.n_envs):
            raise ValueError("the checkpoint is of another PPO: fused_update=%s, obs_dim=%d, n_envs=%d; this one: %s, %d, %d"
                             % (sd["fused_update"], sd["obs_dim"], sd["n_envs"], self.fused_update, self.env.obs_dim, self.env.n_envs))
        if self.fused_update and sd["flat"].numel() != self.flat.numel():
            raise ValueError("the checkpoint's policy has %d parameters, this one %d (another --arch)" % (sd["flat"].numel(), self.flat.numel()))
        self._restore(sd)

    def _load_params(self, sd):
        if self.fused_update:
            self._load_adam_state(sd)
        else:
            self.policy.load_state_dict(sd["policy"])
            self.opt.load_state_dict(sd["opt"])

    def iterate(self):
        obs_b, act_b, logp_b, adv, ret, rew = self.collect()
        stats = self.update(obs_b, act_b, logp_b, adv, ret)
        stats["mean_step_reward"] = float(rew.mean())
        if self.objective is not None:
            stats["objective_terms"] = self.objective.report()["terms"][0]
        if self.track_episodes:
            eps, ret, length = self._episode_stats()
            stats.update(episodes=eps[0], mean_episode_return=ret[0], mean_episode_length=length[0])
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


HYPER_COLS = 8   # a row of `hyper` (include/pcc_policy.h): {lr, clip, ent_coef, gamma, lam, max_grad_norm, 0, 0}
HYPER_NAMES = ("lr", "clip", "ent_coef", "gamma", "lam", "max_grad_norm")   # the columns PopulationPPO.evolve can perturb or bound, by name


def explore_matrix(factors=(0.8, 1.2), explore=("lr", "ent_coef"), bounds=None):
    """The [8][4] rows {factor_lo, factor_hi, min, max} pcc_pbt_evolve takes (include/pcc_policy.h), as a list: the columns
    named in `explore` get `factors`, every other column -- the two reserved ones too -- {1, 1, -inf, +inf}, which inherits
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


def _hyper_columns(members, **named):
    """lr, clip, ent_coef, gamma, lam, max_grad_norm -- each a scalar (a number, a numpy scalar, a 0-dim tensor) or one value per member -- as
    `members` rows of `hyper`."""
    cols = []
    for name in HYPER_NAMES:
        try:
            vals = [float(named[name])] * members
        except (TypeError, ValueError):
            vals = [float(x) for x in named[name]]
        if len(vals) != members:
            raise ValueError("PopulationPPO: %s has %d values for %d members" % (name, len(vals), members))
        cols.append(vals)
    return [list(r) + [0.0] * (HYPER_COLS - len(HYPER_NAMES)) for r in zip(*cols)]


class PopulationPPO(_Trainer):
    """`members` independent PPO learners -- each its own policy, Adam state and hyper-parameters -- on `members` equal slices
    of ONE BatchedNetworkEnv: the env is stepped once per step for the whole batch, and the policy forward, the advantage
    estimation and the optimiser step are each one library call for all members (include/pcc_policy.h: pcc_policy_act_pop,
    pcc_gae_pop, pcc_ppo_minibatch_step_pop), bit-identical to the members run one by one through the single-policy entry
    points.  Seeds for a learning curve, or a sweep over lr / clip / ent_coef / gamma / lam: each is a scalar or one value per
    member.  Member m's policy starts as PPO(seed=seeds[m])'s: like PPO, construction reseeds torch's global generators
    (torch.manual_seed, member by member), so they are left seeded by seeds[-1], and the rollout's noise and the minibatch
    permutations are drawn from the device's from there.  There is no framework path: anything the library has no kernel
    for raises ValueError.
    diagnostics / target_kl / diag_rows: PPO's options, per member: update() adds per-member lists of
    approx_kl, clip_fraction, explained_variance, max_log_ratio, nonfinite and epochs_run.  With target_kl a member whose approximate
    KL after an epoch exceeds 1.5 x target_kl, or is NaN (its parameters have gone non-finite), is stopped for the rest of that
    update: its later minibatches are gradient-only, exactly as an lr == 0 member's are -- its parameters and Adam's moments stay as
    they are -- while the other members go on; Adam's step count stays the population's (it goes on for the stopped member too).  The
    decision is the kernel's: no copy to the host, no synchronise.
    max_grad_norm: PPO's option, a scalar or one limit per member: column 5 of hyper, so a replaced member
    takes its parent's through evolve(), which can perturb or bound it by its name; update() adds per-member lists of grad_norm,
    max_grad_norm_seen, clipped_steps and skipped_steps.  A member whose gradient is not finite skips that step alone; the others
    go on.  None (the default): column 5 stays 0 and the steps are pcc_ppo_minibatch_step_pop's.
    rng="philox": PPO's option, per member: member m draws with the key made from seeds[m], so its numbers do
    not depend on the other members, on their number or on its slot -- it equals PPO(seed=seeds[m], rng="philox") on a handle of its
    own env ids -- and nothing is drawn from torch's generators.
    bootstrap_time_limit: PPO's option: the terminal rows are valued by pcc_policy_act_pop, every member its
    own columns with its own parameters, and pcc_gae_boot_pop reads every member's gamma and lambda.  The option has no state:
    evolve() and the checkpoint's tensors are what they are without it.
    objective: PPO's option: one objective for all members, or a list of one per member -- a sweep over what
    the controllers are trained for.  The weights stay with their slots through evolve(), as the keyed streams do: a replaced member
    goes on with its parent's parameters under its own objective.  evolve(scores=None) ranks the ledger's returns, which under
    different objectives do not compare: it raises then; explicit scores work (for instance the ledger's channel "reward").
    iterate() adds objective_terms, a list of {term: mean weighted term}."""

    def __init__(self, env, members, arch=(32, 16), lr=1e-3, clip=0.2, ent_coef=0.01, gamma=0.99, lam=0.95, seeds=None,
                 epochs=4, minibatch=None, horizon=64, normalize_obs=False, clip_obs=10.0, norm_eps=1e-8, track_episodes=False,
                 normalize_reward=False, clip_reward=10.0, diagnostics=False, target_kl=None, diag_rows=None, max_grad_norm=None,
                 rng="torch", bootstrap_time_limit=False, objective=None):
        members = int(members)
        self._set_rng(env, rng)
        self._set_normalize(env, normalize_obs)
        if members < 1 or members > 1024:
            raise ValueError("PopulationPPO: members = %d (1 .. 1024)" % members)
        self._set_grad_clip(env, max_grad_norm, True, members)
        if int(env.n_envs) % members == 0:   # (else refused below, in the words of before)
            self._set_objective(env, objective, members)
        if len(arch) != 2:
            raise ValueError("PopulationPPO needs a policy of two hidden layers (arch = %r)" % (tuple(arch),))
        if int(env.n_envs) % members != 0:
            raise ValueError("PopulationPPO: %d envs do not divide into %d members" % (env.n_envs, members))
        self.hyper_rows = _hyper_columns(members, lr=lr, clip=clip, ent_coef=ent_coef, gamma=gamma, lam=lam,
                                         max_grad_norm=0.0 if max_grad_norm is None else self.max_grad_norm)
        seeds = list(range(members)) if seeds is None else [int(x) for x in seeds]
        if len(seeds) != members:
            raise ValueError("PopulationPPO: seeds has %d values for %d members" % (len(seeds), members))
        if not isinstance(env, BatchedNetworkEnv) or torch.device(env.device).type != "cuda" or env.n_senders != 1:
            raise ValueError("PopulationPPO needs a BatchedNetworkEnv with one sender on the GPU (no GroupedNetworkEnv)")
        if lib().pcc_ppo_supported(int(env.obs_dim), int(arch[0]), int(arch[1])) != 1:
            raise ValueError("PopulationPPO: the library has no kernels for %d observations x hidden %s (pcc_ppo_supported)"
                             % (env.obs_dim, list(arch)))
        self._set_episodes(env, track_episodes, members)
        self._set_reward_norm(env, normalize_reward, clip_reward, norm_eps, members)
        self._set_diagnostics(env, diagnostics, target_kl, diag_rows, horizon, members)
        self._set_time_limit(env, bootstrap_time_limit, horizon, members)
        self.env, self.members, self.arch = env, members, (int(arch[0]), int(arch[1]))
        self.epochs, self.horizon, self.adam_eps = epochs, horizon, 1e-5
        self.n_member = int(env.n_envs) // members
        dev = env.device
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
        if self.max_grad_norm is not None:
            self.grad_clip = GradClip(self.param_stride, members, dev)
        self._first_obs(members, clip_obs, norm_eps)
        self._make_streams(seeds)
        per_member = self.n_member * horizon
        self.minibatch = min(per_member, max(2048, per_member // 4)) if minibatch is None else int(minibatch)

    def _stream(self):
        return current_stream(self.env.device)

    def _act(self, obs, noise, act, logp, val):
        """The policies on one [N, D] observation row: member m on its slice with its parameters, one launch."""
        N, D = obs.shape
        call("pcc_policy_act_pop", _ptr(obs), N, D, _ptr(self.flat), self.param_stride, self.members, self.arch[0], self.arch[1],
             _ptr(noise), None, _ptr(act), _ptr(logp), _ptr(val), self._stream())

    def _gae(self, rew_b, val_b, done_b, last_v):
        if self.bootstrap_time_limit:   # the terminal rows' values under the parameters as they are now: the rollout's own
            self.time_limit.values(lambda o, v: self._act(o, None, None, None, v))
            return self.time_limit.gae_pop(rew_b, val_b, done_b, last_v, self.hyper)
        T, N = rew_b.shape
        adv, ret = torch.empty_like(rew_b), torch.empty_like(rew_b)
        d8 = done_b.view(torch.uint8)
        call("pcc_gae_pop", _ptr(rew_b), _ptr(val_b), _ptr(d8), _ptr(last_v), T, N, self.members, _ptr(self.hyper), _ptr(adv), _ptr(ret),
             self._stream())
        return adv, ret

    def collect(self, noise=None):
        """One rollout of `horizon` steps of the whole batch: per step pcc_policy_act_pop (every member on its slice) and ONE
        env step; then the last values, the env's flags, and pcc_gae_pop with every member's gamma and lambda.  noise: the
        [horizon, n_envs] standard-normal draws (default: drawn here).  Returns PPO.collect()'s tuple; the value and done rows
        stay in self.val_b / self.done_b.  With rng="philox" the default is every member's keyed stream of this iteration
        (self.iteration advances once per call, whether noise is given or not)."""
        env, T, N = self.env, self.horizon, int(self.env.n_envs)
        if self.rng == "philox":
            self.iteration += 1
        rows = _RolloutRows(self, T, N)
        if noise is None:
            noise = self.streams.noise(T, self.iteration) if self.rng == "philox" else torch.randn((T, N), device=env.device)
        rows.run(env, noise, self._act)
        last_v = torch.empty(N, device=env.device)
        self._act(rows.finish(self), None, None, None, last_v)
        env.check_flags()
        adv, ret = self._gae(rows.rew_gae, rows.val, rows.done, last_v)
        self.val_b, self.done_b = rows.val, rows.done
        return rows.obs[:T], rows.act, rows.logp, adv, ret, rows.rew

    def _reward_gamma(self):
        return self.hyper   # (every member's own gamma, as the device holds it now: column 3)

    def normalise(self, adv):
        return normalise_per_member(adv, self.members)

    def minibatch_step(self, obs_f, act_f, logp_f, adv_f, ret_f, perm, start, count, grad_out=None):
        """One optimiser step of every member on its samples perm[m][start : start + count] (global indices into the flattened
        rollout): two launches (pcc_ppo_minibatch_step_pop).  With target_kl the hyper block it passes is self.diag.hyper_live, which
        update() sets up (begin) and the checks keep: a stopped member's step is gradient-only."""
        if start < 0 or count < 1 or start + count > perm.shape[1]:
            raise ValueError("minibatch [%d, %d) outside a member's rollout" % (start, start + count))
        self.adam_t += 1
        D = obs_f.shape[1]
        if self.grad_clip is not None:   # the same step through the clipped entry: the limits are column 5 of the hyper block
            gc = self.grad_clip
            return call("pcc_ppo_minibatch_step_clip_pop", _ptr(obs_f), _ptr(act_f), _ptr(logp_f), _ptr(adv_f), _ptr(ret_f), _ptr(perm),
                        perm.stride(0), start, count, D, self.arch[0], self.arch[1], _ptr(self.flat), _ptr(self.adam_m),
                        _ptr(self.adam_v), self.param_stride, self.members,
                        _ptr(self.hyper if self.target_kl is None else self.diag.hyper_live), self.adam_t, 0.9, 0.999, self.adam_eps,
                        _ptr(self.scratch), _ptr(gc.grad if grad_out is None else grad_out), _ptr(self.stats_buf), _ptr(gc.hyper_grad),
                        _ptr(gc.clip), gc.clip.stride(0), self._stream())
        call("pcc_ppo_minibatch_step_pop", _ptr(obs_f), _ptr(act_f), _ptr(logp_f), _ptr(adv_f), _ptr(ret_f), _ptr(perm), perm.stride(0),
             start, count, D, self.arch[0], self.arch[1], _ptr(self.flat), _ptr(self.adam_m),
             _ptr(self.adam_v), self.param_stride, self.members,
             _ptr(self.hyper if self.target_kl is None else self.diag.hyper_live), self.adam_t, 0.9, 0.999,
             self.adam_eps, _ptr(self.scratch), _ptr(grad_out), _ptr(self.stats_buf), self._stream())

    def update(self, obs_b, act_b, logp_b, adv, ret, perms=None):
        """`epochs` passes over every member's own samples in minibatches of self.minibatch samples per member.  perms: one
        [members][T * n_m] tensor per epoch (population_permutations; default: drawn here, one draw per epoch -- with rng="philox" every
        member's order of (its key, self.iteration, epoch), and the advantages standardised by the library).  With diagnostics
        every epoch ends with the checks of updiag.UpdateDiagnostics on the rollout's rows (the values are self.val_b, collect()'s)."""
        T, N = adv.shape
        n = T * N
        philox = self.rng == "philox"
        adv_f = (self.streams.standardise(adv.contiguous()) if philox else self.normalise(adv)).reshape(n)
        obs_f, act_f = obs_b.reshape(n, -1).contiguous(), act_b.reshape(n).contiguous()
        logp_f, ret_f = logp_b.reshape(n).contiguous(), ret.reshape(n).contiguous()
        per_member = T * self.n_member
        if self.diagnostics:
            self.diag.begin(self.hyper)
        if self.grad_clip is not None:
            self.grad_clip.begin()
        for e in range(self.epochs):
            perm = perms[e] if perms is not None else (self._order(T, e) if philox else
                                                       population_permutations(T, N, self.members, device=adv.device))
            for i in range(0, per_member, self.minibatch):
                self.minibatch_step(obs_f, act_f, logp_f, adv_f, ret_f, perm, i, min(self.minibatch, per_member - i))
            if self.diagnostics:   # what this epoch did to every member, and who still updates in the next one
                self.diag.check(e + 1, obs_f.view(T, N, -1), act_f, logp_f, ret_f, self.val_b.contiguous(), self.flat, self.param_stride,
                                self.n_params, self.arch, self.hyper, self._kl_limit())
        st = self.stats_buf.tolist()   # of every member's last minibatch
        log_std = [float(x) for x in self.flat[:, (self.n_params - 1) // 2].tolist()]
        ent = [x + 0.5 * (1.0 + math.log(2.0 * math.pi)) for x in log_std]
        out = {"pg": [-r[0] for r in st], "vf": [0.5 * r[1] for r in st], "entropy": ent, "clip_frac": [r[2] for r in st]}
        if self.diagnostics:
            out.update(self.diag.report(self.epochs))
        if self.grad_clip is not None:
            out.update(self.grad_clip.report())
        return out

    def iterate(self):
        """collect() + update(); per-member lists of mean_step_reward, pg, vf, entropy, clip_frac and, with track_episodes, of
        episodes, mean_episode_return and mean_episode_length (the episodes the rollout finished; NaN without one)."""
        obs_b, act_b, logp_b, adv, ret, rew = self.collect()
        stats = self.update(obs_b, act_b, logp_b, adv, ret)
        stats["mean_step_reward"] = rew.reshape(rew.shape[0], self.members, self.n_member).mean(dim=(0, 2)).tolist()
        if self.objective is not None:
            stats["objective_terms"] = self.objective.report()["terms"]
        if self.track_episodes:
            stats["episodes"], stats["mean_episode_return"], stats["mean_episode_length"] = self._episode_stats()
        return stats

    def evolve(self, scores=None, frac=0.25, factors=(0.8, 1.2), explore=("lr", "ent_coef"), bounds=None, seed=0):
        """The step between two generations of population-based training, one launch (pcc_pbt_evolve, include/pcc_policy.h): the
        n_cut = int(frac * members) members with the lowest `scores` (K numbers or a tensor, larger is better, NaN last) each
        take over the parameters, Adam's moments and the hyper-parameters of a member drawn from the best n_cut, and the
        hyper-parameters named in `explore` are multiplied by one of the two `factors` and clamped to `bounds` ({name: (lo, hi)}).
        scores=None (track_episodes only): the ledger's mean finished-episode return since the last such call, read on the device
        (a member without a finished episode scores NaN: last); the ledger's totals are cleared afterwards.
        The draws are Philox's of (seed, self.generation, member): a run repeats and resumes bit for bit.  With rng="philox" the
        learners' keys stay with their slots: a replaced member takes its parent's weights and goes on with its own stream; so do the
        objectives' weights (section 27).  Returns (parent, rank)
        as device int32 tensors -- parent[m] == m for a member that was not replaced -- without synchronising.  The host mirror
        hyper_rows is stale from here on (None): hypers() reads the rows back."""
        if not 0.0 <= frac <= 0.5:
            raise ValueError("evolve: frac = %r (0 .. 0.5: the worst members are replaced from as many of the best)" % (frac,))
        dev = self.env.device
        own = scores is None
        if own:
            if not self.track_episodes:
                raise ValueError("evolve: scores=None takes the episode ledger's mean episode return: PopulationPPO(track_episodes=True)")
            if self.objective is not None and not self.objective.uniform():
                raise ValueError("evolve: scores=None ranks the members by their episode returns, and returns under different objectives "
                                 "do not rank: pass scores (for instance the ledger's channel \"reward\": self.ledger.scores(\"reward\"))")
            scores = self.ledger.scores()
        score = torch.as_tensor(scores).detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        if score.numel() != self.members:
            raise ValueError("evolve: %d scores for %d members" % (score.numel(), self.members))
        ex = torch.tensor(explore_matrix(factors, explore, bounds), dtype=torch.float32, device=dev)
        parent = torch.empty(self.members, dtype=torch.int32, device=dev)
        rank = torch.empty(self.members, dtype=torch.int32, device=dev)
        call("pcc_pbt_evolve", _ptr(score), self.members, int(frac * self.members), _ptr(self.flat), _ptr(self.adam_m), _ptr(self.adam_v),
             self.param_stride, self.n_params, _ptr(self.hyper), _ptr(ex), int(seed) & 0xFFFFFFFFFFFFFFFF,
             self.generation & 0xFFFFFFFF, _ptr(parent), _ptr(rank), self._stream())
        if self.normalize_obs:   # weights without their normaliser are meaningless: a replaced member takes its parent's too
            self.obs_norm.inherit(parent)
        if self.track_episodes:  # a replaced member's finished episodes were another policy's
            self.ledger.inherit(parent)
            if own:
                self.ledger.clear()
        if self.normalize_reward:   # the value network's targets are in its parent's scale
            self.rew_norm.inherit(parent)
        self.generation += 1
        self.hyper_rows = None
        return parent, rank

    def hypers(self):
        """Every member's hyper row as the device holds it now ([members][8] floats, a list).  A synchronise: for logging."""
        return self.hyper.tolist()

    def state_dict(self):
        """Everything the next iterate() depends on (PPO.state_dict's contract): the flat block, Adam's state and step, hyper, the
        observation, the generator states and the env's snapshot; and the generation the next evolve() draws with."""
        sd = {"format": "population-1", "members": self.members, "obs_dim": int(self.env.obs_dim), "n_envs": int(self.env.n_envs),
              "arch": self.arch, "generation": int(self.generation), "hyper": self.hyper.clone()}
        sd.update(self._adam_state())
        sd.update(self._common_state())
        return sd

    def load_state_dict(self, sd):
        """Continue from a state_dict() of a PopulationPPO of the same construction (env configuration, members, arch)."""
        if sd.get("format") != "population-1":
            raise ValueError("not a PopulationPPO.state_dict() of this version")
        mine = (self.members, int(self.env.obs_dim), int(self.env.n_envs), tuple(self.arch))
        theirs = (sd["members"], sd["obs_dim"], sd["n_envs"], tuple(sd["arch"]))
        if mine != theirs:
            raise ValueError("the checkpoint is of another population: (members, obs_dim, n_envs, arch) = %s; this one: %s" % (theirs, mine))
        self._restore(sd)

    def _load_params(self, sd):
        self._load_adam_state(sd)
        self.hyper.copy_(sd["hyper"])
        self.hyper_rows = [[float(x) for x in r] for r in self.hyper.tolist()]
        self.generation = int(sd.get("generation", 0))   # (a checkpoint from before evolve() has none)
