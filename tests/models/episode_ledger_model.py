"""A numpy restatement of the episode ledger's contract (include/pcc_policy.h: pcc_episode_update_pop):
sequential per-env float64 sums in step order, the list of the finished episodes, and the members' totals with their sums
rounded once from the exact sum (math.fsum) -- the reference of the device's sum / sumsq, next to the bound on their error.
tests/test_episodes_cpu.py holds it against a plain Python loop, tests/test_episodes.py holds the device against it."""
import math

import numpy as np

STEP_COLS = 19
U = 2.0 ** -53   # float64's unit roundoff


def channel_rows(reward, steps, cols):
    """x [T][N][C] float64: channel 0 the float32 reward row widened, channel c >= 1 column cols[c - 1] of the step records."""
    reward = np.asarray(reward, dtype=np.float32)
    x = [reward.astype(np.float64)]
    for col in cols:
        x.append(np.asarray(steps, dtype=np.float64)[:, :, col])
    return np.stack(x, axis=2)


class Ledger(object):
    """The buffers of the contract.  episodes[m]: member m's finished episodes since the start, as (env, length, values[C])."""

    def __init__(self, n_envs, members=1, cols=(), totals_stride=None):
        self.N, self.K, self.cols = int(n_envs), int(members), list(cols)
        self.C = 1 + len(self.cols)
        self.stride = 2 + 4 * self.C if totals_stride is None else int(totals_stride)
        self.carry = np.zeros((self.N, self.C))
        self.carry_len = np.zeros(self.N, dtype=np.int32)
        self.last = np.zeros((self.N, self.C))
        self.last_len = np.zeros(self.N, dtype=np.int32)
        self.totals = np.zeros((self.K, self.stride))
        self.episodes = [[] for _ in range(self.K)]

    def update(self, reward, done, steps=None):
        """One call: T steps in order, one float64 addition per env, channel and step; returns the episodes finished in this call,
        per member, and merges them into totals (exact sums, rounded once: see totals_of)."""
        x = channel_rows(reward, steps, self.cols)
        done = np.asarray(done) != 0
        n_m = self.N // self.K
        new = [[] for _ in range(self.K)]
        for t in range(x.shape[0]):
            self.carry = self.carry + x[t]           # one IEEE addition per element
            self.carry_len = self.carry_len + 1
            for i in np.nonzero(done[t])[0]:
                new[i // n_m].append((int(i), int(self.carry_len[i]), self.carry[i].copy()))
                self.last[i] = self.carry[i]
                self.last_len[i] = self.carry_len[i]
                self.carry[i] = 0.0
                self.carry_len[i] = 0
        for m in range(self.K):
            if new[m]:
                self.episodes[m] += new[m]
                self.totals[m, :2 + 4 * self.C] = merge_row(self.totals[m], new[m], self.C)
        return new


def merge_row(row, eps, C):
    """A totals row {episodes, steps, per channel sum, sumsq, min, max} with the episodes `eps` merged in: counts, min and max
    exact, sum and sumsq the exactly rounded sum of the row's value and the episodes' (any order the device takes is within
    sum_bound of it)."""
    out = np.array(row[:2 + 4 * C], dtype=np.float64)
    had = row[0] > 0
    out[0] = row[0] + len(eps)
    out[1] = row[1] + sum(e[1] for e in eps)
    for c in range(C):
        v = [float(e[2][c]) for e in eps]
        out[2 + 4 * c] = math.fsum([row[2 + 4 * c]] + v)
        out[3 + 4 * c] = math.fsum([row[3 + 4 * c]] + [a * a for a in v])
        out[4 + 4 * c] = min(v + ([row[4 + 4 * c]] if had else []))
        out[5 + 4 * c] = max(v + ([row[5 + 4 * c]] if had else []))
    return out


def sum_bounds(eps, C, prior=None):
    """The allowed |sum - want| and |sumsq - want| per channel for a member whose E episodes `eps` were added, in any order, and
    merged with an existing row: E * 2^-52 * sum|v| (and sum v^2) -- the first-order bound (E - 1) * 2^-53 * sum|v| of any
    summation order, doubled for the merge.  prior: a totals row that was not zero before the first of `eps` came in -- its sum
    and sumsq count as one more term each."""
    E = len(eps) + (0 if prior is None else 1)
    b_sum, b_sq = [], []
    for c in range(C):
        v = [float(e[2][c]) for e in eps]
        b_sum.append(E * 2.0 * U * math.fsum([abs(a) for a in v] + ([abs(prior[2 + 4 * c])] if prior is not None else [])))
        b_sq.append(E * 2.0 * U * math.fsum([a * a for a in v] + ([abs(prior[3 + 4 * c])] if prior is not None else [])))
    return b_sum, b_sq


def plain_loop(reward, done, steps, cols, carry=None, carry_len=None):
    """The same thing as a plain Python loop over every env, listing every episode: [(env, end step, length, values[C])], and the
    carry that is left."""
    T, N = np.asarray(reward).shape
    C = 1 + len(cols)
    out = []
    left, left_len = np.zeros((N, C)), np.zeros(N, dtype=np.int32)
    for i in range(N):
        acc = [0.0] * C if carry is None else [float(v) for v in carry[i]]
        n = 0 if carry_len is None else int(carry_len[i])
        for t in range(T):
            acc[0] = acc[0] + float(np.float32(reward[t][i]))
            for c in range(1, C):
                acc[c] = acc[c] + float(steps[t][i][cols[c - 1]])
            n += 1
            if done[t][i]:
                out.append((i, t, n, list(acc)))
                acc, n = [0.0] * C, 0
        left[i], left_len[i] = acc, n
    return out, left, left_len
