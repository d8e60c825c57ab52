"""Keyed random streams of the learners on the device (include/pcc_policy.h: pcc_rollout_noise_pop, pcc_sample_order_pop,
pcc_adv_standardise_pop): the rollout's standard normals, every epoch's minibatch order and the standardised
advantages of rng="philox" (ppo.PPO, ppo.PopulationPPO).  Every learner owns a 64-bit key made from its seed, and what it draws is a
pure function of (key, iteration, step or epoch, its own local sample index): a learner repeats whatever runs beside it, and nothing
is taken from torch's generators.  There is no framework path: the HIP library does the work or the call raises."""
import torch

from .env import _ptr
from .native import call, current_stream, lib

_M64 = 0xFFFFFFFFFFFFFFFF


def key_from_seed(seed):
    """A learner's 64-bit key: the splitmix64 finaliser (Steele, Lea and Flood 2014) of seed + the golden-ratio increment -- seeds
    0, 1, 2, ... give keys that differ in about half of their bits."""
    z = (int(seed) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _as_int64(key):
    return key - (1 << 64) if key >= (1 << 63) else key   # (torch has no uint64 arithmetic: the same 64 bits as int64)


class LearnerStreams(object):
    """keys int64 [members] on the device (the bits of the uint64 keys), member m owning the columns m * n_envs / members ... of
    every [T][n_envs] row.  noise(), order() and standardise() are each one library call for all members; moments [members][2]
    float64 holds {mean, var} of the last standardise()."""

    def __init__(self, seeds, n_envs, device="cuda:0", keys=None):
        self.host_keys = [int(k) & _M64 for k in keys] if keys is not None else [key_from_seed(s) for s in seeds]
        self.members, self.n_envs = len(self.host_keys), int(n_envs)
        if not 1 <= self.members <= 1024 or self.n_envs < 1 or self.n_envs % self.members != 0:
            raise ValueError("LearnerStreams: %d envs do not divide into %d members (1 .. 1024)" % (self.n_envs, self.members))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("LearnerStreams runs HIP kernels: it needs a GPU device (device=%r); there is no CPU path" % (device,))
        self.n_member = self.n_envs // self.members
        self.keys = torch.tensor([_as_int64(k) for k in self.host_keys], dtype=torch.int64, device=self.device)
        self.moments = torch.zeros((self.members, 2), dtype=torch.float64, device=self.device)
        self._scratch = None

    def _steps(self, T, what):
        T = int(T)
        if lib().pcc_adv_standardise_scratch_doubles(T, self.n_envs, self.members) < 0:
            raise ValueError("LearnerStreams.%s: %d steps of %d envs are outside the library's domain" % (what, T, self.n_envs))
        return T

    def noise(self, T, iteration, out=None, words=None):
        """[T][n_envs] float32 standard normals of rollout `iteration`: one launch.  words: a uint32-sized [T][n_envs] int32 tensor
        that takes the raw Philox words (for tests of the layout)."""
        T = self._steps(T, "noise")
        if out is None:
            out = torch.empty((T, self.n_envs), dtype=torch.float32, device=self.device)
        for x, dt in ((out, torch.float32), (words, torch.int32)):
            if x is not None and not (x.is_cuda and x.dtype == dt and x.is_contiguous() and tuple(x.shape) == (T, self.n_envs)):
                raise ValueError("LearnerStreams.noise: expected a contiguous %s [%d][%d] on the GPU, got %s %s"
                                 % (dt, T, self.n_envs, tuple(x.shape), x.dtype))
        call("pcc_rollout_noise_pop", _ptr(out), _ptr(words), T, self.n_envs, self.members, _ptr(self.keys), int(iteration) & 0xFFFFFFFF,
             current_stream(self.device))
        return out

    def order(self, T, iteration, epoch, out=None):
        """[members][T * n_envs / members] int64: row m a permutation of member m's own samples as indices into the flattened [T *
        n_envs] rollout arrays (ppo.population_sample_index) -- what pcc_ppo_minibatch_step_pop takes as `perm`: one launch, no sort."""
        T = self._steps(T, "order")
        n = T * self.n_member
        if out is None:
            out = torch.empty((self.members, n), dtype=torch.int64, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.int64 and out.dim() == 2 and out.shape[0] == self.members and out.shape[1] >= n
                  and out.stride(1) == 1):
            raise ValueError("LearnerStreams.order: expected int64 rows [%d][>= %d] on the GPU, got %s %s"
                             % (self.members, n, tuple(out.shape), out.dtype))
        call("pcc_sample_order_pop", _ptr(out), out.stride(0) if self.members > 1 else out.shape[1], T, self.n_envs, self.members,
             _ptr(self.keys), int(iteration) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, current_stream(self.device))
        return out

    def standardise(self, adv, out=None):
        """out[T][n_envs] = float32((a - mean) / (std + 1e-8)) per member over its own columns, float64 throughout (PPO.update's
        formula): one library call, three launches.  out may be adv itself; default: a new tensor."""
        if not (torch.is_tensor(adv) and adv.is_cuda and adv.dtype == torch.float32 and adv.is_contiguous() and adv.dim() == 2
                and adv.shape[0] >= 1 and adv.shape[1] == self.n_envs):
            raise ValueError("LearnerStreams.standardise: expected contiguous float32 rows [T][%d] on the GPU, got %s %s"
                             % (self.n_envs, tuple(getattr(adv, "shape", ())), getattr(adv, "dtype", type(adv))))
        T = self._steps(adv.shape[0], "standardise")
        if out is None:
            out = torch.empty_like(adv)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == adv.shape):
            raise ValueError("LearnerStreams.standardise: the output must be contiguous float32 rows of the input's shape")
        need = lib().pcc_adv_standardise_scratch_doubles(T, self.n_envs, self.members)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float64, device=self.device)
        call("pcc_adv_standardise_pop", _ptr(adv), T, self.n_envs, self.members, _ptr(self._scratch), _ptr(self.moments), _ptr(out),
             current_stream(self.device))
        return out

    def state_dict(self):
        return {"keys": list(self.host_keys), "n_envs": self.n_envs}

    def load_state_dict(self, sd):
        keys = [int(k) & _M64 for k in sd["keys"]]
        if (len(keys), int(sd["n_envs"])) != (self.members, self.n_envs):
            raise ValueError("the checkpoint's streams are of another shape: (members, n_envs) = %s; this one: %s"
                             % ((len(keys), int(sd["n_envs"])), (self.members, self.n_envs)))
        self.host_keys = keys
        self.keys.copy_(torch.tensor([_as_int64(k) for k in keys], dtype=torch.int64))
