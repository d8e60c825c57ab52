"""Reward objectives on the device (include/pcc_policy.h: pcc_reward_objective_pop): the reward rows of a
rollout recomputed from its float64 step records under per-member weights over six of their metrics -- what a controller is trained
for as an option, one library call for all members of a population, no change to any env kernel.  With the reference weights
(RewardObjective.DEFAULT) the rows are the env's own reward rows bit for bit.  There is no framework path: the HIP library does the
work or the call raises."""
import math
import types
from collections.abc import Mapping

import torch

from .env import _ptr
from .native import PCC_STEP_COLS, call, current_stream, lib

# the terms in the order of the PCC_OBJ_* enum, and the metric each one weighs (native.STEP_COLUMNS)
TERMS = ("throughput", "latency", "loss", "latency_inflation", "latency_ratio", "send_rate")
TERM_COLUMNS = ("recv rate", "avg latency", "loss ratio", "sent latency inflation", "latency ratio", "send rate")
N_TERMS = len(TERMS)


def weight_row(spec, who="RewardObjective"):
    """One member's weights as a list of N_TERMS floats from a dict of term names (a name left out weighs 0) or a sequence of
    N_TERMS numbers.  Unknown names and weights that are not finite raise ValueError."""
    if isinstance(spec, Mapping):
        unknown = [k for k in spec if k not in TERMS]
        if unknown:
            raise ValueError("%s: no term %s (one of %s)" % (who, ", ".join(repr(k) for k in unknown), ", ".join(TERMS)))
        row = [float(spec.get(name, 0.0)) for name in TERMS]
    else:
        try:
            row = [float(x) for x in spec]
        except (TypeError, ValueError):
            raise ValueError("%s: weights are a dict of term names or %d numbers, got %r" % (who, N_TERMS, spec))
        if len(row) != N_TERMS:
            raise ValueError("%s: %d weights for the %d terms (%s)" % (who, len(row), N_TERMS, ", ".join(TERMS)))
    for name, x in zip(TERMS, row):
        if not math.isfinite(x):
            raise ValueError("%s: the weight of %r is %r (finite numbers only)" % (who, name, x))
    return row


def _is_number(x):
    try:
        float(x)
        return not isinstance(x, (str, bytes))
    except (TypeError, ValueError):
        return False


def weight_rows(spec, members, who="RewardObjective"):
    """`members` rows of weights from one dict or sequence of numbers (every member the same) or one dict or sequence per member;
    None: the reference objective."""
    if spec is None:
        spec = RewardObjective.DEFAULT
    if torch.is_tensor(spec):
        spec = spec.tolist()
    if isinstance(spec, Mapping):
        return [weight_row(spec, who) for _ in range(members)]
    entries = list(spec)
    if entries and all(_is_number(x) for x in entries):
        return [weight_row(entries, who) for _ in range(members)]
    if len(entries) != members:
        raise ValueError("%s: %d per-member objectives for %d members" % (who, len(entries), members))
    return [weight_row(e, who) for e in entries]


def parse(text):
    """'throughput=10,latency=-1000,loss=-2000' as a dict of weights; with ';' between members, a list of such dicts (the examples'
    --objective)."""
    def one(part):
        out = {}
        for item in part.split(","):
            if not item.strip():
                continue
            name, sep, value = item.partition("=")
            if not sep:
                raise ValueError("objective: %r is not name=weight" % item)
            try:
                out[name.strip()] = float(value)
            except ValueError:
                raise ValueError("objective: the weight of %r is %r (a number)" % (name.strip(), value))
        return out
    parts = [one(p) for p in text.split(";")]
    return parts[0] if len(parts) == 1 else parts


class RewardObjective(object):
    """weights [members][6] float64 on the device (and self.rows, the same numbers on the host): member m owns the columns m * n_envs
    / members ... of every [T][n_envs] row.  sums [members][7] float64: the last apply()'s per-member sums of the six weighted terms
    before the scale and of the float32 rewards."""

    DEFAULT = types.MappingProxyType({"throughput": 10.0, "latency": -1e3, "loss": -2e3})   # the env's own reward

    def __init__(self, n_envs, members=1, weights=None, device="cuda:0"):
        self.n_envs, self.members = int(n_envs), int(members)
        if not 1 <= self.members <= 1024 or self.n_envs < 1 or self.n_envs % self.members != 0:
            raise ValueError("RewardObjective: %d envs do not divide into %d members (1 .. 1024)" % (self.n_envs, self.members))
        self.rows = weight_rows(weights, self.members)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("RewardObjective runs HIP kernels: it needs a GPU device (device=%r); there is no CPU path" % (device,))
        self.n_member = self.n_envs // self.members
        self.weights = torch.tensor(self.rows, dtype=torch.float64, device=self.device)
        self.sums = torch.zeros((self.members, N_TERMS + 1), dtype=torch.float64, device=self.device)
        self.samples = 0   # T * n_member of the last apply(): what report() divides by
        self._scratch = None

    def uniform(self):
        """Whether every member has the same weights."""
        return all(r == self.rows[0] for r in self.rows)

    def apply(self, steps_b, out=None):
        """The reward rows [T][N] float32 of the step records steps_b [T][N][19] (or [T][N][1][19]) float64, contiguous on the GPU,
        and self.sums of them: one library call, two launches, no synchronise.  out: the rows to write into; default: a new tensor."""
        if torch.is_tensor(steps_b) and steps_b.dim() == 4 and steps_b.shape[2] == 1:
            steps_b = steps_b.reshape(steps_b.shape[0], steps_b.shape[1], steps_b.shape[3])
        if not (torch.is_tensor(steps_b) and steps_b.is_cuda and steps_b.dtype == torch.float64 and steps_b.is_contiguous()
                and steps_b.dim() == 3 and steps_b.shape[0] >= 1 and tuple(steps_b.shape[1:]) == (self.n_envs, PCC_STEP_COLS)):
            raise ValueError("RewardObjective: expected contiguous float64 step records [T][%d][%d] on the GPU, got %s %s"
                             % (self.n_envs, PCC_STEP_COLS, tuple(getattr(steps_b, "shape", ())), getattr(steps_b, "dtype", type(steps_b))))
        T = int(steps_b.shape[0])
        if out is None:
            out = torch.empty((T, self.n_envs), dtype=torch.float32, device=self.device)
        elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                  and tuple(out.shape) == (T, self.n_envs)):
            raise ValueError("RewardObjective: out is float32 [%d][%d], contiguous on the GPU" % (T, self.n_envs))
        need = lib().pcc_objective_scratch_doubles(T, self.n_envs, self.members)
        if need < 0:
            raise ValueError("RewardObjective.apply: records of %s are outside the library's domain" % (tuple(steps_b.shape),))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float64, device=self.device)
        call("pcc_reward_objective_pop", _ptr(steps_b), T, self.n_envs, self.members, _ptr(self.weights), _ptr(out), _ptr(self.sums),
             _ptr(self._scratch), current_stream(self.device))
        self.samples = T * self.n_member
        return out

    def report(self):
        """Of the last apply(), per member: {"terms": [{name: mean weighted term}, ...], "reward": [mean reward, ...]} -- the terms
        before the scale, those with weight 0 left out.  A synchronise: for logging."""
        if self.samples < 1:
            raise ValueError("RewardObjective.report: nothing applied yet")
        rows, n = self.sums.tolist(), float(self.samples)
        return {"terms": [{name: s / n for name, s, w in zip(TERMS, r, wr) if w != 0.0} for r, wr in zip(rows, self.rows)],
                "reward": [r[N_TERMS] / n for r in rows]}

    def state_dict(self):
        return {"n_envs": self.n_envs, "members": self.members, "terms": list(TERMS), "weights": self.weights.clone()}

    def load_state_dict(self, sd):
        mine, theirs = (self.n_envs, self.members, list(TERMS)), (int(sd["n_envs"]), int(sd["members"]), list(sd["terms"]))
        if mine != theirs:
            raise ValueError("the checkpoint's reward objective is of another shape: (n_envs, members, terms) = %s; this one: %s" % (theirs, mine))
        rows = [weight_row(r, "the checkpoint's reward objective") for r in sd["weights"].tolist()]
        self.rows = rows
        self.weights.copy_(torch.tensor(rows, dtype=torch.float64))
