"""A numpy restatement of pcc_ppo_minibatch_step_clip_pop's own part (include/pcc_policy.h): the sum of squares
in the stated order, the state and coefficient rules, and Adam in float64 with the error bounds the float32 kernel is held to.  The
Adam part restates adam_step64 / _assert_adam of tests/test_policy_numerics.py (restated, not imported: this file stands alone), with
the learning rate as an argument; u = 2^-24."""
import math

import numpy as np

LANES = 256
U = 2.0 ** -24
TINY = 2.0 ** -149     # the smallest float32 subnormal: what one float32 operation can lose to gradual underflow
NORM_EPS = 1e-6        # torch.nn.utils.clip_grad_norm_'s
F32 = lambda x: float(np.float32(x))
B1, B2, EPS = F32(0.9), F32(0.999), F32(1e-5)
APPLIED, CLIPPED, SKIPPED, GRAD_ONLY = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------------- the ordered sum
def lane_sums(g):
    """x[j], j < 256: lane j's float64 sum of g[p]^2 over p = j, j + 256, ... in increasing p, from 0.0."""
    sq = np.asarray(g).astype(np.float64).reshape(-1)
    sq = sq * sq
    rows = (sq.size + LANES - 1) // LANES
    pad = np.zeros(rows * LANES, dtype=np.float64)   # (a lane without a term adds + 0.0: the sums keep their bits)
    pad[:sq.size] = sq
    x = np.zeros(LANES, dtype=np.float64)
    for r in pad.reshape(rows, LANES):               # one add per term, in increasing p
        x = x + r
    return x


def tree(x):
    """for s = 128, 64, ..., 1: x[j] += x[j + s] for j < s; returns x[0]."""
    x = np.array(x, dtype=np.float64)
    s = LANES // 2
    while s >= 1:
        x[:s] = x[:s] + x[s:2 * s]
        s //= 2
    return float(x[0])


def ordered_sumsq(g):
    with np.errstate(invalid="ignore", over="ignore"):
        return tree(lane_sums(g))


# -------------------------------------------------------------------------------------------- state and coefficient
def decide(sumsq, lr, limit):
    """(state, c as a float32, norm): lr and limit are the member's hyper[0] and hyper[5] as float32 values."""
    with np.errstate(invalid="ignore"):
        norm = float(np.sqrt(np.float64(sumsq)))
    lr, limit = np.float32(lr), np.float32(limit)
    if lr == 0.0:
        return GRAD_ONLY, np.float32(1.0), norm
    if not math.isfinite(sumsq):
        return SKIPPED, np.float32(1.0), norm
    c64 = np.float64(limit) / (np.float64(norm) + NORM_EPS)
    if limit > 0.0 and c64 < 1.0:
        return CLIPPED, np.float32(c64), norm
    return APPLIED, np.float32(1.0), norm


def accumulate(row, sumsq, lr, limit):
    """One call's effect on a row {sumsq, norm, c, state, steps, clipped_steps, skipped_steps, max_norm_seen}; returns the state."""
    state, c, norm = decide(sumsq, lr, limit)
    row[0], row[1], row[2], row[3] = sumsq, norm, float(c), float(state)
    row[4] += 1.0 if state in (APPLIED, CLIPPED) else 0.0
    row[5] += 1.0 if state == CLIPPED else 0.0
    row[6] += 1.0 if state == SKIPPED else 0.0
    if norm > row[7]:      # fmax: a NaN norm does not enter it
        row[7] = norm
    return state


# ------------------------------------------------------------------------------------------------------------ Adam
def adam_step64(t, g, m0, v0, lr):
    """torch.optim.Adam's step in float64 from float32 inputs and float32-rounded constants: (m, v, step(m, v))."""
    g, m0, v0, lr = (np.asarray(a, dtype=np.float64) for a in (g, m0, v0, lr))
    m = B1 * m0 + (1.0 - B1) * g
    v = B2 * v0 + (1.0 - B2) * g * g
    return m, v, lambda m_, v_: lr / (1.0 - B1 ** t) * np.asarray(m_, np.float64) / (np.sqrt(np.asarray(v_, np.float64)) / math.sqrt(1.0 - B2 ** t) + EPS)


def adam_errors(t, g, before, after, lr):
    """One float32 step held to the float64 restatement: the moments from g and the moments before, the parameter step from the
    float32 moments after.  Returns the largest (error / bound) of m, v and the step: each must be <= 1.  The bounds are
    _assert_adam's (4u on the two products and the sum of m; 6u on v; 8u + the bias corrections' share on the step and u on the
    parameter's own rounding), plus one subnormal for an operation that underflows."""
    (m0, v0, p0), (m1, v1, p1) = [[np.asarray(a, dtype=np.float64) for a in s] for s in (before, after)]
    g = np.asarray(g, dtype=np.float64)
    m64, v64, step = adam_step64(t, g, m0, v0, lr)
    b_m = 4 * U * (np.abs(B1 * m0) + np.abs((1.0 - B1) * g)) + TINY
    b_v = 6 * U * v64 + TINY
    want = step(m1, v1)
    rel = 8 * U + 2 * U * B1 ** t / (1.0 - B1 ** t) + U * B2 ** t / (1.0 - B2 ** t)
    b_p = rel * np.abs(want) + U * np.maximum(np.abs(p0), np.abs(p1)) + TINY
    return (float((np.abs(m1 - m64) / b_m).max()), float((np.abs(v1 - v64) / b_v).max()), float((np.abs(p0 - p1 - want) / b_p).max()))


def clipped_step64(t, g, m0, v0, p0, lr, limit):
    """The whole rule in float64 on a float64 gradient -- norm, coefficient, Adam -- for the comparison with torch: (p, m, v, state)."""
    g = np.asarray(g, dtype=np.float64)
    state, _, norm = decide(ordered_sumsq(g), 1.0, limit)
    c = float(limit) / (norm + NORM_EPS) if state == CLIPPED else 1.0
    m, v, step = adam_step64(t, g * c, m0, v0, lr)
    return p0 - step(m, v), m, v, state
