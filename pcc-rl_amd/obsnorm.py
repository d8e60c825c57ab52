"""Observation normalisation on the device (include/pcc_policy.h: pcc_obs_stats_update_pop, pcc_obs_normalise_pop; DESIGN.md
section 19): running per-member, per-feature mean and variance of the raw observation rows in float64, and the standardised,
clipped rows the policy kernels read -- stable-baselines' VecNormalize / baselines-ppo1's ob_rms, as one library call for all
members of a population.  There is no framework path: the HIP library does the work or the call raises."""
import torch

from .env import _ptr
from .native import call, current_stream, lib


class ObsNormalizer(object):
    """stats [members][1 + 2 D] float64 {count, mean, m2}, norm [members][2 D] float32 {shift, scale}: member m owns the columns
    m * N / members ... of every [N][D] row.  A fresh normaliser has shift 0 and scale 1: the identity, with the clip."""

    def __init__(self, obs_dim, members=1, clip=10.0, eps=1e-8, device="cuda:0"):
        self.obs_dim, self.members, self.clip, self.eps = int(obs_dim), int(members), float(clip), float(eps)
        if not 1 <= self.obs_dim <= 128 or not 1 <= self.members <= 1024:
            raise ValueError("ObsNormalizer: obs_dim = %d (1 .. 128), members = %d (1 .. 1024)" % (self.obs_dim, self.members))
        if not self.clip > 0.0 or not self.eps >= 0.0:
            raise ValueError("ObsNormalizer: clip = %r (> 0), eps = %r (>= 0)" % (clip, eps))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("ObsNormalizer runs HIP kernels: it needs a GPU device (device=%r); there is no CPU path" % (device,))
        D = self.obs_dim
        self.stat_stride = 1 + 2 * D
        self.stats = torch.zeros((self.members, self.stat_stride), dtype=torch.float64, device=self.device)
        self.norm = torch.cat([torch.zeros((self.members, D)), torch.ones((self.members, D))], dim=1).to(self.device).contiguous()
        self._scratch = None

    def _rows(self, x, dims):
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == dims and x.shape[-1] == self.obs_dim):
            raise ValueError("ObsNormalizer: expected contiguous float32 rows of %d observations on the GPU, got %s %s"
                             % (self.obs_dim, tuple(x.shape), x.dtype))
        if x.shape[-2] % self.members != 0:
            raise ValueError("ObsNormalizer: %d envs do not divide into %d members" % (x.shape[-2], self.members))
        return x

    def normalise(self, raw_rows, out=None):
        """out[N][D] = clamp((raw_rows - shift) * scale, -clip, clip) with every member's row of norm: one launch.  out may be
        raw_rows itself; default: a new tensor."""
        raw_rows = self._rows(raw_rows, 2)
        out = torch.empty_like(raw_rows) if out is None else self._rows(out, 2)
        N, D = raw_rows.shape
        call("pcc_obs_normalise_pop", _ptr(raw_rows), N, D, self.members, _ptr(self.norm), self.clip, _ptr(out), current_stream(self.device))
        return out

    def update(self, raw_b):
        """Merge the moments of raw_b[T][N][D] into every member's statistics and rewrite norm: two launches."""
        raw_b = self._rows(raw_b, 3)
        T, N, D = raw_b.shape
        need = lib().pcc_obs_stats_scratch_doubles(T, N, D, self.members)
        if need < 0:
            raise ValueError("ObsNormalizer.update: a batch of %s is outside the library's domain" % (tuple(raw_b.shape),))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float64, device=self.device)
        call("pcc_obs_stats_update_pop", _ptr(raw_b), T, N, D, self.members, _ptr(self.stats), self.stat_stride, _ptr(self.norm),
             self.eps, _ptr(self._scratch), current_stream(self.device))

    def member(self, m):
        """(shift, scale, clip) of member m, the tensors on the CPU: what export.export_policy(obs_norm=...) takes.  A synchronise."""
        D = self.obs_dim
        row = self.norm[m].cpu()
        return row[:D].clone(), row[D:].clone(), self.clip

    def inherit(self, parent):
        """Member m takes the stats and norm rows of member parent[m] (PopulationPPO.evolve's returned tensor; parent[m] == m
        keeps its own): an index-select on the device, no synchronise."""
        idx = parent.to(device=self.device, dtype=torch.int64)
        self.stats.copy_(self.stats.index_select(0, idx))
        self.norm.copy_(self.norm.index_select(0, idx))

    def state_dict(self):
        return {"obs_dim": self.obs_dim, "members": self.members, "clip": self.clip, "eps": self.eps,
                "stats": self.stats.clone(), "norm": self.norm.clone()}

    def load_state_dict(self, sd):
        mine, theirs = (self.obs_dim, self.members), (int(sd["obs_dim"]), int(sd["members"]))
        if mine != theirs:
            raise ValueError("the checkpoint's normaliser is of another shape: (obs_dim, members) = %s; this one: %s" % (theirs, mine))
        self.clip, self.eps = float(sd["clip"]), float(sd["eps"])
        self.stats.copy_(sd["stats"])
        self.norm.copy_(sd["norm"])
