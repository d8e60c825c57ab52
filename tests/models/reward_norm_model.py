"""Reward normalisation, restated in numpy (include/pcc_policy.h: pcc_return_stats_update_pop, pcc_reward_normalise_pop; DESIGN.md
section 22): the walk that the header fixes bit for bit, the moments through the restatement of tests/test_obs_norm_cpu.py
(batch_moments, chan_merge, moment_bounds), scale from stats, the normalise step -- and kernel_order_moments, the summation order
of csrc/pcc_rewnorm.hip itself (lane over T, a tree over the workgroup, the partials in index order), which the CPU tests hold
against the two-pass."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from test_obs_norm_cpu import batch_moments, chan_merge, moment_bounds  # noqa: E402,F401

THREADS, WAVE = 256, 64
REWARD_KINDS = ("unit", "offset", "wide")   # N(0, 1), N(-50, 1), N(0, 3e3)


def make_rewards(kind, shape, rng):
    loc, sd = {"unit": (0.0, 1.0), "offset": (-50.0, 1.0), "wide": (0.0, 3e3)}[kind]
    return (loc + sd * rng.standard_normal(shape)).astype(np.float32)


DONE_KINDS = ("none", "every", "bernoulli", "last", "fixed")


def make_done(kind, shape, rng):
    T, N = shape
    d = np.zeros(shape, dtype=np.uint8)
    if kind == "every":
        d[:] = 1
    elif kind == "bernoulli":
        d = (rng.random(shape) < 0.1).astype(np.uint8)
    elif kind == "last":
        d[T - 1] = 1
    elif kind == "fixed":
        d[T // 2] = 3   # (any value != 0 ends the episode)
    return d


def member_gammas(gamma, K):
    """One float32 gamma per member from a number or K numbers."""
    g = np.asarray(gamma, dtype=np.float32).reshape(-1)
    return np.repeat(g, K) if g.size == 1 else g


def walk(reward, done, gammas, carry):
    """(samples [T][N] float64, carry [N] float64 after the call): R = R * (double)gamma_m + (double)r, the sample, R = 0 on done."""
    reward, done = np.asarray(reward, dtype=np.float32), np.asarray(done)
    T, N = reward.shape
    g = np.repeat(np.asarray(gammas, dtype=np.float32), N // len(gammas)).astype(np.float64)
    R = np.array(carry, dtype=np.float64)
    samples = np.empty((T, N), dtype=np.float64)
    for t in range(T):
        R = R * g + reward[t].astype(np.float64)
        samples[t] = R
        R = np.where(done[t] != 0, 0.0, R)
    return samples, R


def member_samples(samples, m, K):
    """Member m's samples [T][N] as one column [n][1] (what batch_moments takes)."""
    n_m = samples.shape[1] // K
    return samples[:, m * n_m:(m + 1) * n_m].reshape(-1, 1)


def update_stats(stats, samples, K):
    """stats [K][stride] after the update with these samples, by the two-pass and Chan's merge; the padding stays."""
    out = np.array(stats, dtype=np.float64)
    for m in range(K):
        n, mean, m2 = chan_merge((out[m, 0], out[m, 1:2].copy(), out[m, 2:3].copy()), batch_moments(member_samples(samples, m, K)))
        out[m, 0], out[m, 1], out[m, 2] = n, mean[0], m2[0]
    return out


def scale_from_stats(stats, eps):
    """scale [K] float32 from stats: float64 arithmetic, rounded to float32 once."""
    stats = np.asarray(stats, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0 / np.sqrt(stats[:, 2] / stats[:, 0] + np.float64(eps))).astype(np.float32)


def normalise(reward, scale, K, clip):
    """out [T][N] float32: two float32 operations per element, member m's columns with scale[m]."""
    reward = np.asarray(reward, dtype=np.float32)
    s = np.repeat(np.asarray(scale, dtype=np.float32), reward.shape[1] // K)
    c = np.float32(clip)
    with np.errstate(over="ignore", invalid="ignore"):   # (a product beyond float32 is +-inf, and clipped)
        return np.fmin(np.fmax(reward * s, -c), c).astype(np.float32)


# ----------------------------------------------------------------------------------- the kernels' own order of the sums
def _chan(a, b):
    """chan_merge of csrc/pcc_rewnorm.hip on arrays: an empty side leaves the other as it is."""
    (na, ma, qa), (nb, mb, qb) = a, b
    with np.errstate(divide="ignore", invalid="ignore"):
        n = na + nb
        d = mb - ma
        mean = ma + d * nb / n
        m2 = qa + qb + d * d * na * nb / n
    keep_a, take_b = nb == 0.0, (na == 0.0) & (nb != 0.0)
    return (np.where(keep_a, na, np.where(take_b, nb, n)), np.where(keep_a, ma, np.where(take_b, mb, mean)),
            np.where(keep_a, qa, np.where(take_b, qb, m2)))


def kernel_order_moments(samples):
    """(n, mean, m2) of one member's samples [T][n_m] in the order of return_walk_kernel and return_merge_kernel: lane = env sums
    {x - k, (x - k)^2}, k its first sample, in step order; the 64 lanes of a wavefront by Chan's formula in a down-shuffle tree;
    the 4 wavefronts of a workgroup in index order; 256 sub-lanes each sum a contiguous range of the workgroups' partials in index
    order, division-free; a halving tree over the sub-lanes."""
    x = np.asarray(samples, dtype=np.float64)
    T, n_m = x.shape
    groups = (n_m + THREADS - 1) // THREADS
    lanes = groups * THREADS
    k = np.zeros(lanes)
    k[:n_m] = x[0]
    s, q = np.zeros(lanes), np.zeros(lanes)
    for t in range(T):
        d = x[t] - k[:n_m]
        s[:n_m] += d
        q[:n_m] += d * d
    cnt = np.where(np.arange(lanes) < n_m, float(T), 0.0)
    dev = q - s * s / T
    cur = (cnt.reshape(-1, WAVE), np.where(cnt > 0, k + s / T, 0.0).reshape(-1, WAVE), np.where(dev > 0.0, dev, 0.0).reshape(-1, WAVE))
    for d in (32, 16, 8, 4, 2, 1):   # lane j takes lane j + d in (a lane past the end reads itself: never part of lane 0's tree)
        src = np.minimum(np.arange(WAVE) + d, WAVE - 1)
        src = np.where(np.arange(WAVE) + d < WAVE, src, np.arange(WAVE))
        cur = _chan(cur, tuple(c[:, src] for c in cur))
    waves = tuple(c[:, 0].reshape(groups, THREADS // WAVE) for c in cur)
    part = tuple(c[:, 0] for c in waves)
    for w in range(1, THREADS // WAVE):
        part = _chan(part, tuple(c[:, w] for c in waves))
    pn, pm, pq = part                                        # [groups] each: what goes to scratch
    per = (groups + THREADS - 1) // THREADS
    kk = pm[0]
    a = np.zeros((4, THREADS))
    for tid in range(THREADS):
        for g in range(min(tid * per, groups), min(tid * per + per, groups)):
            c, d = pn[g], pm[g] - kk
            a[0, tid] += c
            a[1, tid] += c * d
            a[2, tid] += c * (d * d)
            a[3, tid] += pq[g]
    half = THREADS // 2
    while half >= 1:
        a[:, :half] += a[:, half:2 * half]
        half //= 2
    nb, s1, s2, s3 = a[:, 0]
    between = s2 - s1 * s1 / nb
    return nb, kk + s1 / nb, s3 + (between if between > 0.0 else 0.0)
