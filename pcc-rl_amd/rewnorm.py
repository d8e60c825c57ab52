"""Reward normalisation on the device (include/pcc_policy.h: pcc_return_stats_update_pop, pcc_reward_normalise_pop; DESIGN.md
section 22): the running per-member variance of every env's discounted return in float64, and the reward rows divided by its square
root and clipped -- the norm_reward half of stable-baselines' VecNormalize, as one library call for all members of a population.
There is no framework path: the HIP library does the work or the call raises."""
import torch

from .env import _ptr
from .native import call, current_stream, lib

HYPER_COLS, HYPER_GAMMA = 8, 3   # a row of the population's `hyper` block, and its gamma column (include/pcc_policy.h)


class RewardNormalizer(object):
    """stats [members][3] float64 {count, mean, m2} of the discounted returns, scale [members] float32, ret_carry [n_envs] float64
    (every env's running discounted return): member m owns the columns m * n_envs / members ... of every [T][n_envs] row.  A fresh
    normaliser has scale 1 and ret_carry 0: the identity, with the clip."""

    def __init__(self, n_envs, members=1, clip=10.0, eps=1e-8, device="cuda:0"):
        self.n_envs, self.members, self.clip, self.eps = int(n_envs), int(members), float(clip), float(eps)
        if not 1 <= self.members <= 1024 or self.n_envs < 1 or self.n_envs % self.members != 0:
            raise ValueError("RewardNormalizer: %d envs do not divide into %d members (1 .. 1024)" % (self.n_envs, self.members))
        if not self.clip > 0.0 or not self.eps >= 0.0:
            raise ValueError("RewardNormalizer: clip = %r (> 0), eps = %r (>= 0)" % (clip, eps))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("RewardNormalizer runs HIP kernels: it needs a GPU device (device=%r); there is no CPU path" % (device,))
        self.stat_stride = 3
        self.stats = torch.zeros((self.members, self.stat_stride), dtype=torch.float64, device=self.device)
        self.scale = torch.ones(self.members, dtype=torch.float32, device=self.device)
        self.ret_carry = torch.zeros(self.n_envs, dtype=torch.float64, device=self.device)
        self._scratch = None

    def _rows(self, x, what, dtypes):
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype in dtypes and x.is_contiguous() and x.dim() == 2 and x.shape[0] >= 1
                and x.shape[1] == self.n_envs):
            raise ValueError("RewardNormalizer: expected contiguous %s rows [T][%d] on the GPU, got %s %s"
                             % (what, self.n_envs, tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x))))
        return x

    def update(self, rew_b, done_b, hyper_or_gamma):
        """The raw rows of T steps, in step order, into every env's running return and every member's statistics, and scale
        rewritten: one library call, two launches.  rew_b [T][N] float32, done_b [T][N] bool or uint8; hyper_or_gamma: the
        population's [members][8] float32 block on the device (column 3: gamma), or, with one member, a number."""
        rew_b = self._rows(rew_b, "float32 reward", (torch.float32,))
        done_b = self._rows(done_b, "bool / uint8 done", (torch.bool, torch.uint8))
        if done_b.dtype == torch.bool:
            done_b = done_b.view(torch.uint8)
        T = rew_b.shape[0]
        if done_b.shape[0] != T:
            raise ValueError("RewardNormalizer.update: %d reward rows, %d done rows" % (T, done_b.shape[0]))
        need = lib().pcc_return_scratch_doubles(T, self.n_envs, self.members)
        if need < 0:
            raise ValueError("RewardNormalizer.update: a batch of %s is outside the library's domain" % (tuple(rew_b.shape),))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float64, device=self.device)
        if torch.is_tensor(hyper_or_gamma) and hyper_or_gamma.dim() == 2:
            h = hyper_or_gamma
            if not (h.is_cuda and h.dtype == torch.float32 and h.is_contiguous() and tuple(h.shape) == (self.members, HYPER_COLS)):
                raise ValueError("RewardNormalizer.update: expected the contiguous float32 hyper block [%d][%d] on the GPU, got %s %s"
                                 % (self.members, HYPER_COLS, tuple(h.shape), h.dtype))
            call("pcc_return_stats_update_pop", _ptr(rew_b), _ptr(done_b), T, self.n_envs, self.members, _ptr(h), _ptr(self.ret_carry),
                 _ptr(self.stats), self.stat_stride, _ptr(self.scale), self.eps, _ptr(self._scratch), current_stream(self.device))
            return
        if self.members != 1:
            raise ValueError("RewardNormalizer.update: %d members need the hyper block (one gamma per member), not a number" % self.members)
        call("pcc_return_stats_update", _ptr(rew_b), _ptr(done_b), T, self.n_envs, float(hyper_or_gamma), _ptr(self.ret_carry),
             _ptr(self.stats), _ptr(self.scale), self.eps, _ptr(self._scratch), current_stream(self.device))

    def normalise(self, rew_b, out=None):
        """out[T][N] = clamp(rew_b * scale, -clip, clip) with every member's scale: one launch.  out may be rew_b itself; default:
        a new tensor."""
        rew_b = self._rows(rew_b, "float32 reward", (torch.float32,))
        out = torch.empty_like(rew_b) if out is None else self._rows(out, "float32 output", (torch.float32,))
        if out.shape != rew_b.shape:
            raise ValueError("RewardNormalizer.normalise: %d reward rows, %d output rows" % (rew_b.shape[0], out.shape[0]))
        call("pcc_reward_normalise_pop", _ptr(rew_b), rew_b.shape[0], self.n_envs, self.members, _ptr(self.scale), self.clip, _ptr(out),
             current_stream(self.device))
        return out

    def inherit(self, parent):
        """Member m takes the stats and scale rows of member parent[m] (PopulationPPO.evolve's returned tensor; parent[m] == m
        keeps its own): an index-select on the device, no synchronise.  ret_carry belongs to the envs, which stay with their
        slice: it is left alone."""
        idx = parent.to(device=self.device, dtype=torch.int64)
        self.stats.copy_(self.stats.index_select(0, idx))
        self.scale.copy_(self.scale.index_select(0, idx))

    def state_dict(self):
        return {"n_envs": self.n_envs, "members": self.members, "clip": self.clip, "eps": self.eps, "stats": self.stats.clone(),
                "scale": self.scale.clone(), "ret_carry": self.ret_carry.clone()}

    def load_state_dict(self, sd):
        mine, theirs = (self.n_envs, self.members), (int(sd["n_envs"]), int(sd["members"]))
        if mine != theirs:
            raise ValueError("the checkpoint's reward normaliser is of another shape: (n_envs, members) = %s; this one: %s" % (theirs, mine))
        self.clip, self.eps = float(sd["clip"]), float(sd["eps"])
        self.stats.copy_(sd["stats"])
        self.scale.copy_(sd["scale"])
        self.ret_carry.copy_(sd["ret_carry"])
