"""The episode ledger on the device (include/pcc_policy.h: pcc_episode_update_pop): what every episode
returned -- stable-baselines' ep_rew_mean / ep_len_mean -- exact, per member, deterministic, from the reward and done rows a
rollout already holds, and, with step records, per-episode totals of any of their columns.  One library call per rollout for
all members, nothing copied to the host until summary() is asked for.  There is no framework path: the HIP library does the
work or the call raises."""
import ctypes

import torch

from .env import _ptr
from .native import PCC_STEP_COLS, STEP_COLUMNS, call, current_stream, lib

# short names of step-record columns, next to native.STEP_COLUMNS' own
_ALIASES = {"latency_ratio": "latency ratio", "loss_ratio": "loss ratio", "send_rate": "send rate", "recv_rate": "recv rate",
            "avg_latency": "avg latency", "send_ratio": "send ratio"}


def column_index(channel):
    """The step-record column of a channel given by name (native.STEP_COLUMNS, blanks or underscores) or by index."""
    if isinstance(channel, str):
        name = _ALIASES.get(channel, channel)
        name = name if name in STEP_COLUMNS else name.replace("_", " ")
        if name not in STEP_COLUMNS:
            raise ValueError("EpisodeLedger: no step-record column %r (one of %s)" % (channel, ", ".join(STEP_COLUMNS)))
        return STEP_COLUMNS.index(name)
    col = int(channel)
    if not 0 <= col < PCC_STEP_COLS:
        raise ValueError("EpisodeLedger: step-record column %d (0 .. %d)" % (col, PCC_STEP_COLS - 1))
    return col


class EpisodeLedger(object):
    """carry [N][C] float64 and carry_len [N] int32: every env's running episode; last / last_len: its last finished one;
    totals [members][2 + 4 C] float64: row m is {episodes, steps, then per channel sum, sumsq, min, max} of the channel totals of
    the episodes member m's envs (the columns m * N / members ...) finished since clear().  Channel 0 is the float32 reward row;
    `channels` names step-record columns for channels 1 ... (at most 7)."""

    def __init__(self, n_envs, members=1, channels=(), device="cuda:0"):
        self.n_envs, self.members = int(n_envs), int(members)
        self.columns = [column_index(c) for c in channels]
        self.names = ["reward_f32"] + [STEP_COLUMNS[c] for c in self.columns]
        self.n_channels = 1 + len(self.columns)
        if not 1 <= self.members <= 1024 or self.n_envs < 1 or self.n_envs % self.members != 0:
            raise ValueError("EpisodeLedger: %d envs do not divide into %d members (1 .. 1024)" % (self.n_envs, self.members))
        if self.n_channels > 8:
            raise ValueError("EpisodeLedger: %d step-record channels (at most 7)" % len(self.columns))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("EpisodeLedger runs HIP kernels: it needs a GPU device (device=%r); there is no CPU path" % (device,))
        N, C, dev = self.n_envs, self.n_channels, self.device
        self._cols = (ctypes.c_int32 * max(1, len(self.columns)))(*self.columns)
        self.totals_stride = 2 + 4 * C
        self.carry = torch.zeros((N, C), dtype=torch.float64, device=dev)
        self.carry_len = torch.zeros(N, dtype=torch.int32, device=dev)
        self.last = torch.zeros((N, C), dtype=torch.float64, device=dev)
        self.last_len = torch.zeros(N, dtype=torch.int32, device=dev)
        self._totals = torch.zeros((self.members, self.totals_stride), dtype=torch.float64, device=dev)
        need = lib().pcc_episode_scratch_doubles(N, self.members, C)
        if need < 0:
            raise ValueError("EpisodeLedger: (n_envs, members, channels) = (%d, %d, %d) is outside the library's domain" % (N, self.members, C))
        self._scratch = torch.empty(need, dtype=torch.float64, device=dev)

    def _rows(self, x, what, dtypes, tail=()):
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype in dtypes and x.is_contiguous() and x.dim() == 2 + len(tail)
                and x.shape[1] == self.n_envs and tuple(x.shape[2:]) == tuple(tail)):
            raise ValueError("EpisodeLedger: expected contiguous %s rows [T][%d]%s on the GPU, got %s %s"
                             % (what, self.n_envs, "".join("[%d]" % d for d in tail), tuple(getattr(x, "shape", ())), getattr(x, "dtype", type(x))))
        return x

    def update(self, rew_b, done_b, steps_b=None):
        """The rows of T steps, in step order, into the ledger: one library call, two launches.  rew_b [T][N] float32, done_b
        [T][N] bool or uint8, steps_b [T][N][19] (or [T][N][1][19]) float64 -- step_many's steps_out -- when the ledger has
        step-record channels."""
        rew_b = self._rows(rew_b, "float32 reward", (torch.float32,))
        done_b = self._rows(done_b, "bool / uint8 done", (torch.bool, torch.uint8))
        if done_b.dtype == torch.bool:
            done_b = done_b.view(torch.uint8)
        T = rew_b.shape[0]
        if done_b.shape[0] != T or T < 1:
            raise ValueError("EpisodeLedger.update: %d reward rows, %d done rows" % (T, done_b.shape[0]))
        if self.columns:
            if steps_b is None:
                raise ValueError("EpisodeLedger.update: this ledger's channels %s need the step records (steps_b)" % (self.names[1:],))
            if steps_b.dim() == 4 and steps_b.shape[2] == 1:
                steps_b = steps_b.reshape(steps_b.shape[0], steps_b.shape[1], steps_b.shape[3])
            steps_b = self._rows(steps_b, "float64 step-record", (torch.float64,), (PCC_STEP_COLS,))
            if steps_b.shape[0] != T:
                raise ValueError("EpisodeLedger.update: %d reward rows, %d step-record rows" % (T, steps_b.shape[0]))
        else:
            steps_b = None
        call("pcc_episode_update_pop", _ptr(rew_b), _ptr(done_b), _ptr(steps_b), self._cols, self.n_channels, T, self.n_envs,
             self.members, _ptr(self.carry), _ptr(self.carry_len), _ptr(self.last), _ptr(self.last_len), _ptr(self._totals),
             self.totals_stride, _ptr(self._scratch), current_stream(self.device))

    def totals(self):
        """The device tensor [members][2 + 4 C] itself (not a copy)."""
        return self._totals

    def scores(self, channel=0):
        """Device float64 [members]: the mean finished-episode total of `channel` since clear(), NaN for a member without a
        finished episode -- what PopulationPPO.evolve takes (pcc_pbt_evolve ranks NaN last).  No synchronise."""
        c = self._channel(channel)
        eps = self._totals[:, 0]
        return torch.where(eps > 0, self._totals[:, 2 + 4 * c] / eps, torch.full_like(eps, float("nan")))

    def _channel(self, channel):
        if isinstance(channel, str) and channel in self.names:
            return self.names.index(channel)
        if isinstance(channel, str):
            col = column_index(channel)
            if col not in self.columns:
                raise ValueError("EpisodeLedger: %r is not one of this ledger's channels %s" % (channel, self.names))
            return 1 + self.columns.index(col)
        c = int(channel)
        if not 0 <= c < self.n_channels:
            raise ValueError("EpisodeLedger: channel %d (0 .. %d)" % (c, self.n_channels - 1))
        return c

    def summary(self, totals=None):
        """Per member, on the host: {"episodes": [...], "mean_length": [...], "channels": {name: {"mean", "std", "min", "max"}}},
        each a list of `members` numbers; NaN where a member has no finished episode.  std is the population's, sqrt(sumsq / E -
        mean^2).  The ledger's only synchronise (totals: a tensor of the same layout instead of the ledger's own)."""
        return summarise((self._totals if totals is None else totals).tolist(), self.names)

    def clear(self):
        """Zero the totals; the running episodes go on."""
        self._totals.zero_()

    def inherit(self, parent):
        """After PopulationPPO.evolve: envs stay with their slice and the running episode belongs to the env, so carry and last
        are left alone; the totals row of a replaced member (parent[m] != m) is cleared -- its episodes were another policy's.
        On the device, no synchronise."""
        idx = parent.to(device=self.device, dtype=torch.int64)
        keep = idx == torch.arange(self.members, device=self.device)
        self._totals.copy_(torch.where(keep.unsqueeze(1), self._totals, torch.zeros_like(self._totals)))

    def state_dict(self):
        return {"n_envs": self.n_envs, "members": self.members, "columns": list(self.columns), "carry": self.carry.clone(),
                "carry_len": self.carry_len.clone(), "last": self.last.clone(), "last_len": self.last_len.clone(),
                "totals": self._totals.clone()}

    def load_state_dict(self, sd):
        mine, theirs = (self.n_envs, self.members, list(self.columns)), (int(sd["n_envs"]), int(sd["members"]), [int(c) for c in sd["columns"]])
        if mine != theirs:
            raise ValueError("the checkpoint's episode ledger is of another shape: (n_envs, members, columns) = %s; this one: %s" % (theirs, mine))
        for name, dst in (("carry", self.carry), ("carry_len", self.carry_len), ("last", self.last), ("last_len", self.last_len),
                          ("totals", self._totals)):
            if tuple(sd[name].shape) != tuple(dst.shape) or sd[name].dtype != dst.dtype:
                raise ValueError("the checkpoint's episode ledger: %s is %s %s, expected %s %s"
                                 % (name, tuple(sd[name].shape), sd[name].dtype, tuple(dst.shape), dst.dtype))
            dst.copy_(sd[name])


def summarise(rows, names):
    """EpisodeLedger.summary() of totals rows given as lists (host arithmetic only)."""
    nan = float("nan")
    out = {"episodes": [int(r[0]) for r in rows], "mean_length": [r[1] / r[0] if r[0] > 0 else nan for r in rows], "channels": {}}
    for c, name in enumerate(names):
        ch = {"mean": [], "std": [], "min": [], "max": []}
        for r in rows:
            e, (s, q, lo, hi) = r[0], r[2 + 4 * c:6 + 4 * c]
            if e > 0:
                mean = s / e
                ch["mean"].append(mean)
                ch["std"].append(max(q / e - mean * mean, 0.0) ** 0.5)
                ch["min"].append(lo)
                ch["max"].append(hi)
            else:
                for k in ch:
                    ch[k].append(nan)
        out["channels"][name] = ch
    return out
