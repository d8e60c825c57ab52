"""Time-limit bootstrapping on the device (include/pcc_policy.h: pcc_terminal_obs, pcc_gae_boot, pcc_gae_boot_pop; DESIGN.md section
26).  Every episode of this env ends at max_steps and nowhere else: a done is a truncation, and the advantage estimation may
bootstrap from the value of the observation the episode ended in (Pardo et al. 2018) instead of from zero.  With auto_reset the env
overwrites that observation with the next episode's first one; terminal_observations() rebuilds it, bit for bit, from the rows a
rollout already holds.  There is no framework path for the rebuild: the HIP library does the work or the call raises."""
import ctypes

import torch

from .env import _ptr
from .metrics import METRIC_NAMES, metric_info
from .native import PCC_STEP_COLS, call, current_stream

METRIC_COL0 = 7   # a step record's first metric column (native.STEP_COLUMNS: "send rate"); metric id i is column 7 + i
MAX_FEATURES = 16


def _of(env):
    """The env whose features and max_steps describe the batch: a GroupedNetworkEnv's groups are all alike."""
    return env.groups[0] if hasattr(env, "groups") else env


def feature_columns(env):
    """(cols, scales) of the env's features: the step-record column of each and the scale its observation entry is divided by."""
    ids = [int(i) for i in _of(env).feature_ids]
    return [METRIC_COL0 + i for i in ids], [float(metric_info(METRIC_NAMES[i])[2]) for i in ids]


def slots(T, max_steps):
    """ceil(T / max_steps): an upper bound on the dones of one env in T consecutive rows.  Two dones of an env are never fewer than
    max_steps rows apart -- an episode ends when its step counter reaches max_steps and at no other time, and a masked reset only
    sets the counter back to zero, which postpones the next done -- so rows t .. t + max_steps - 1 hold at most one, and T rows
    split into ceil(T / max_steps) such windows."""
    T, max_steps = int(T), int(max_steps)
    if T < 1 or max_steps < 1:
        raise ValueError("slots: T = %d, max_steps = %d (both >= 1)" % (T, max_steps))
    return (T + max_steps - 1) // max_steps


def _check(env, obs_b, steps_b, done_b):
    e = _of(env)
    if e.n_senders != 1:
        raise ValueError("terminal observations need one sender per env (n_senders = %d): the rows are [T][n_envs]" % e.n_senders)
    N, D = int(env.n_envs), int(e.obs_dim)
    T = int(done_b.shape[0]) if torch.is_tensor(done_b) and done_b.dim() >= 1 else 0
    ok = lambda x, dtypes, numel: (torch.is_tensor(x) and x.is_cuda and x.dtype in dtypes and x.is_contiguous() and x.numel() == numel)
    if T < 1 or not ok(done_b, (torch.bool, torch.uint8), T * N):
        raise ValueError("terminal observations: expected contiguous bool / uint8 done rows [T][%d] on the GPU" % N)
    if not torch.is_tensor(obs_b) or obs_b.dim() < 1 or obs_b.shape[0] not in (T, T + 1) or not ok(obs_b, (torch.float32,), obs_b.shape[0] * N * D):
        raise ValueError("terminal observations: expected contiguous float32 observation rows [T (+ 1)][%d][%d] on the GPU" % (N, D))
    if not ok(steps_b, (torch.float64,), T * N * PCC_STEP_COLS):
        raise ValueError("terminal observations: expected contiguous float64 step records [T][%d][%d] on the GPU" % (N, PCC_STEP_COLS))
    return T, N, D


def terminal_observations(env, obs_b, steps_b, done_b, n_slots=None, out=None):
    """The terminal observations of one rollout, for a trainer of the caller's own: obs_b [T (+ 1)][N][H*F] float32 -- the raw rows
    the env wrote, row t what it showed before step t --, steps_b [T][N][19] float64 (env.rollout / step_many / step_into's
    steps_out) and done_b [T][N] bool or uint8, all contiguous on the env's device.  Returns (term_obs [n_slots][N][H*F] float32,
    term_count [N] int32): the k-th done of env i, in step order, fills term_obs[k][i] with the observation the env would have shown
    after that step had it not been reset -- the row's entries from F on, then the new monitor interval's features, each the step
    record's metric divided by its scale in float64 and rounded to float32 once, as the env does --; a slot an env did not reach is
    zeros; term_count[i] counts every done of env i, also those beyond n_slots, which are not stored.
    n_slots None: ceil(T / env.max_steps), which no env exceeds (slots()).  out: (term_obs, term_count) to write into.  One launch,
    no synchronise."""
    T, N, D = _check(env, obs_b, steps_b, done_b)
    e = _of(env)
    n_slots = slots(T, e.max_steps) if n_slots is None else int(n_slots)
    if n_slots < 1:
        raise ValueError("terminal observations: n_slots = %d (>= 1)" % n_slots)
    cols, scales = feature_columns(env)
    F = len(cols)
    if not 1 <= F <= MAX_FEATURES:
        raise ValueError("terminal observations: %d features (1 .. %d)" % (F, MAX_FEATURES))
    dev = obs_b.device
    if out is None:
        out = (torch.empty((n_slots, N, D), dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev))
    term_obs, term_count = out
    if not (term_obs.is_cuda and term_obs.dtype == torch.float32 and term_obs.is_contiguous() and term_obs.numel() == n_slots * N * D
            and term_count.is_cuda and term_count.dtype == torch.int32 and term_count.is_contiguous() and term_count.numel() == N):
        raise ValueError("terminal observations: out is (float32 [%d][%d][%d], int32 [%d]), contiguous on the GPU" % (n_slots, N, D, N))
    d8 = done_b.view(torch.uint8) if done_b.dtype == torch.bool else done_b
    call("pcc_terminal_obs", _ptr(obs_b), _ptr(steps_b), _ptr(d8), T, N, D // F, F, (ctypes.c_int32 * F)(*cols),
         (ctypes.c_double * F)(*scales), n_slots, _ptr(term_obs), _ptr(term_count), current_stream(dev))
    return term_obs, term_count


class TimeLimitBootstrap(object):
    """What PPO / PopulationPPO(bootstrap_time_limit=True) hold: the buffers of one horizon -- term_obs [n_slots][N][D] (the raw
    terminal rows), term_in (the rows the value network reads: term_obs itself, or with an observation normaliser its rows), term_val
    [n_slots][N], term_count [N] -- and the calls, in the order of a rollout: terminal() once the rows are complete, values() with
    the rollout's own parameters, then gae() / gae_pop().  n_slots = slots(horizon, env.max_steps).  No state outlives a rollout:
    nothing of it goes into a checkpoint."""

    def __init__(self, env, horizon, members=1):
        e = _of(env)
        self.device = torch.device(env.device)
        if self.device.type != "cuda":
            raise ValueError("bootstrap_time_limit=True runs HIP kernels: it needs the env on the GPU (device=%r); there is no CPU path"
                             % (env.device,))
        if e.n_senders != 1:
            raise ValueError("bootstrap_time_limit=True needs one sender per env (n_senders = %d): the rows are [T][n_envs]" % e.n_senders)
        self.env, self.T, self.N, self.D, self.members = env, int(horizon), int(env.n_envs), int(e.obs_dim), int(members)
        self.n_slots = slots(self.T, e.max_steps)
        self.term_obs = torch.empty((self.n_slots, self.N, self.D), dtype=torch.float32, device=self.device)
        self.term_in = self.term_obs
        self.term_val = torch.empty((self.n_slots, self.N), dtype=torch.float32, device=self.device)
        self.term_count = torch.empty(self.N, dtype=torch.int32, device=self.device)

    def terminal(self, obs_b, steps_b, done_b, norm=None):
        """The terminal rows of this rollout; norm: the observation normaliser whose rows the policy read during it (its statistics
        as they were frozen for the rollout: call this before they are updated), one normalise launch per slot."""
        terminal_observations(self.env, obs_b, steps_b, done_b, self.n_slots, out=(self.term_obs, self.term_count))
        if norm is None:
            self.term_in = self.term_obs
        else:
            if self.term_in is self.term_obs:
                self.term_in = torch.empty_like(self.term_obs)
            for k in range(self.n_slots):
                norm.normalise(self.term_obs[k], self.term_in[k])
        return self.term_in

    def values(self, value_of):
        """term_val[k] = value_of(term_in[k], out row) for every slot: the caller's deterministic policy forward, value output alone."""
        for k in range(self.n_slots):
            value_of(self.term_in[k], self.term_val[k])
        return self.term_val

    def _rows(self, rew_b, val_b, done_b, last_v):
        T, N = rew_b.shape
        if (T, N) != (self.T, self.N):
            raise ValueError("TimeLimitBootstrap: rows of %s, made for (%d, %d)" % ((T, N), self.T, self.N))
        d8 = done_b.contiguous()
        d8 = d8.view(torch.uint8) if d8.dtype == torch.bool else d8
        return rew_b.contiguous(), val_b.contiguous(), d8, last_v.contiguous().float(), torch.empty_like(rew_b), torch.empty_like(rew_b)

    def gae(self, rew_b, val_b, done_b, last_v, gamma, lam):
        """pcc_gae_boot on the rollout's rows with term_val / term_count as they stand: (adv, ret)."""
        rew, val, d8, last_v, adv, ret = self._rows(rew_b, val_b, done_b, last_v)
        call("pcc_gae_boot", _ptr(rew), _ptr(val), _ptr(d8), _ptr(last_v), _ptr(self.term_val), _ptr(self.term_count), self.n_slots,
             self.T, self.N, gamma, lam, _ptr(adv), _ptr(ret), current_stream(self.device))
        return adv, ret

    def gae_pop(self, rew_b, val_b, done_b, last_v, hyper):
        """pcc_gae_boot_pop: every member's gamma and lambda from the population's hyper block."""
        rew, val, d8, last_v, adv, ret = self._rows(rew_b, val_b, done_b, last_v)
        call("pcc_gae_boot_pop", _ptr(rew), _ptr(val), _ptr(d8), _ptr(last_v), _ptr(self.term_val), _ptr(self.term_count), self.n_slots,
             self.T, self.N, self.members, _ptr(hyper), _ptr(adv), _ptr(ret), current_stream(self.device))
        return adv, ret
