"""Reward objectives, restated in numpy (include/pcc_policy.h: pcc_reward_objective_pop): the reward of a
sample -- float64, the terms in index order, a zero weight skips its column, the first included term starts the sum, the scale, one
cast -- and the per-member sums in the summation order the header states (lane over T, a down tree over the wavefront, the four
wavefronts in index order, the workgroups' partials in contiguous ranges, a halving tree over 256 sub-lanes).  pairwise_sums is a
second, equally valid order: the CPU tests use it to show that they check the order and not just the value."""
import numpy as np

THREADS, WAVE, MERGE_LANES = 256, 64, 256
STEP_COLS, COL_REWARD, METRIC_COL0 = 19, 6, 7
TERMS = ("throughput", "latency", "loss", "latency_inflation", "latency_ratio", "send_rate")
# the metric id of each term (include/pcc_sim.h: PCC_M_*): recv rate, avg latency, loss ratio, sent latency inflation, latency
# ratio, send rate
TERM_METRICS = (1, 4, 5, 7, 10, 0)
TERM_COLS = tuple(METRIC_COL0 + m for m in TERM_METRICS)
RATE_TERMS = (0, 5)              # divided by the bits of a packet after the product
PACKET_BITS = 12000.0
REWARD_SCALE = 0.001
N_TERMS = len(TERMS)
DEFAULT = (10.0, -1e3, -2e3, 0.0, 0.0, 0.0)


def member_weights(weights, K):
    """[K][6] float64 from one row or K rows."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim == 1:
        w = np.tile(w, (K, 1))
    assert w.shape == (K, N_TERMS)
    return w


def terms(steps, weights, K=1):
    """(terms [6][T][N] float64 -- 0.0 for a term left out --, acc [T][N] float64, reward [T][N] float32) of the records steps
    [T][N][19] under K members' weights."""
    steps = np.asarray(steps, dtype=np.float64)
    T, N, _ = steps.shape
    n_m = N // K
    w = member_weights(weights, K)
    out = np.zeros((N_TERMS, T, N), dtype=np.float64)
    acc = np.zeros((T, N), dtype=np.float64)
    for m in range(K):
        sl = slice(m * n_m, (m + 1) * n_m)
        first = True
        for k in range(N_TERMS):
            if w[m, k] == 0.0:
                continue                                  # (the column is never read)
            term = w[m, k] * steps[:, sl, TERM_COLS[k]]
            if k in RATE_TERMS:
                term = term / PACKET_BITS
            out[k][:, sl] = term
            acc[:, sl] = term if first else acc[:, sl] + term
            first = False
    return out, acc, (acc * REWARD_SCALE).astype(np.float32)


def reward(steps, weights, K=1):
    return terms(steps, weights, K)[2]


def _lane_sums(x):
    """[T][n] -> [n]: every lane its T values in step order from +0.0."""
    s = np.zeros(x.shape[1], dtype=np.float64)
    for t in range(x.shape[0]):
        s = s + x[t]
    return s


def _tree(x, width):
    """x[j] += x[j + d] for j < d, d = width / 2, ..., 1, over the last axis (of length width); returns x[..., 0]."""
    x = np.array(x, dtype=np.float64)
    d = width // 2
    while d >= 1:
        x[..., :d] = x[..., :d] + x[..., d:2 * d]
        d //= 2
    return x[..., 0]


def kernel_order_sum(x):
    """The sum of one member's values x [T][n_m] in the order of csrc/pcc_objective.hip."""
    T, n_m = x.shape
    G = (n_m + THREADS - 1) // THREADS
    lanes = np.zeros(G * THREADS, dtype=np.float64)
    lanes[:n_m] = _lane_sums(x)                                       # (idle lanes hold 0.0)
    waves = _tree(lanes.reshape(G, THREADS // WAVE, WAVE), WAVE)      # [G][4]
    part = waves[:, 0]
    for wv in range(1, THREADS // WAVE):
        part = part + waves[:, wv]                                    # the four wavefronts in index order
    per = (G + MERGE_LANES - 1) // MERGE_LANES
    sub = np.zeros(MERGE_LANES, dtype=np.float64)
    for j in range(MERGE_LANES):
        for g in range(min(j * per, G), min(j * per + per, G)):
            sub[j] = sub[j] + part[g]
    return _tree(sub, MERGE_LANES)


def pairwise_sum(x):
    """Another valid order: the lanes as above, then numpy's pairwise sum over the lanes."""
    return np.sum(_lane_sums(x))


def sums(steps, weights, K=1, order=kernel_order_sum):
    """[K][7] float64: per member the sums of the six weighted terms before the scale and of the float32 rewards."""
    tr, _, rew = terms(steps, weights, K)
    T, N = rew.shape
    n_m = N // K
    out = np.zeros((K, N_TERMS + 1), dtype=np.float64)
    for m in range(K):
        sl = slice(m * n_m, (m + 1) * n_m)
        for k in range(N_TERMS):
            out[m, k] = order(tr[k][:, sl])
        out[m, N_TERMS] = order(rew[:, sl].astype(np.float64))
    return out


def make_steps(T, N, seed):
    """Synthetic records in the workload's ranges: rates up to 1e7 bit/s, latencies of tens of milliseconds, loss in [0, 1),
    inflation around 0, ratios from 1 up; the other columns are filled too (counters, clocks)."""
    rng = np.random.default_rng(seed)
    s = rng.random((T, N, STEP_COLS)) * 100.0
    s[..., METRIC_COL0 + 0] = rng.random((T, N)) * 1e7            # send rate
    s[..., METRIC_COL0 + 1] = rng.random((T, N)) * 1e7            # recv rate
    s[..., METRIC_COL0 + 4] = 0.01 + rng.random((T, N)) * 0.3     # avg latency
    s[..., METRIC_COL0 + 5] = rng.random((T, N)) * (rng.random((T, N)) < 0.5)   # loss ratio: half of them exactly 0
    s[..., METRIC_COL0 + 7] = rng.standard_normal((T, N)) * 0.05  # sent latency inflation
    s[..., METRIC_COL0 + 10] = 1.0 + rng.random((T, N)) * 4.0     # latency ratio
    return s
