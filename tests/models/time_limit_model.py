"""Numpy restatements of time-limit bootstrapping (include/pcc_policy.h: pcc_terminal_obs, pcc_gae_boot).
Plain loops over envs and steps: slow, and meant to be read next to the header."""
import numpy as np

STEP_COLS = 19
METRIC_COL0 = 7                       # a step record's first metric column: metric id i is column 7 + i
SCALES = {0: 1e7, 1: 1e7}             # pcc_metric_info's scale of the two rates; every other metric: 1


def feature_columns(feature_ids):
    """(cols, scales) of the env's feature ids."""
    return [METRIC_COL0 + int(i) for i in feature_ids], [SCALES.get(int(i), 1.0) for i in feature_ids]


def slots(T, max_steps):
    return -(-int(T) // int(max_steps))


def terminal_row(obs_row, step_row, F, cols, scales):
    """The observation after a step from the one before it (obs_row [H F] float32, oldest monitor interval first) and the step's
    record (step_row [19] float64): the entries from F on, then every new feature -- a float64 division, one cast to float32."""
    obs_row = np.asarray(obs_row, dtype=np.float32)
    new = np.empty(F, dtype=np.float32)
    for f in range(F):
        new[f] = np.float32(np.float64(step_row[cols[f]]) / np.float64(scales[f]))
    return np.concatenate([obs_row[F:], new])


def terminal_obs(obs, steps, done, F, cols, scales, n_slots):
    """obs [T (+ 1)][N][H F] float32, steps [T][N][19] float64, done [T][N] -> (term_obs [n_slots][N][H F] float32, term_count [N]
    int32): the k-th done of env i in step order fills slot k; a slot without one is zeros; a done beyond n_slots is counted only."""
    T, N = done.shape
    HF = obs.shape[-1]
    term = np.zeros((n_slots, N, HF), dtype=np.float32)
    count = np.zeros(N, dtype=np.int32)
    for i in range(N):
        for t in range(T):
            if done[t, i]:
                if count[i] < n_slots:
                    term[count[i], i] = terminal_row(obs[t, i], steps[t, i], F, cols, scales)
                count[i] += 1
    return term, count


def gae_boot(rew, val, done, last_val, term_val, term_count, gamma, lam):
    """pcc_gae_boot for one member: float32 scalars, the kernel's operations in its order.  term_val [n_slots][N]; term_val None:
    pcc_gae (a done multiplies the next value and the running sum by 0)."""
    T, N = rew.shape
    f = np.float32
    gamma, lam = f(gamma), f(lam)
    adv, ret = np.empty((T, N), dtype=np.float32), np.empty((T, N), dtype=np.float32)
    n_slots = 0 if term_val is None else term_val.shape[0]
    for i in range(N):
        next_v, run = f(last_val[i]), f(0.0)
        c = 0 if term_val is None else int(term_count[i])
        for t in range(T - 1, -1, -1):
            v, r = f(val[t, i]), f(rew[t, i])
            if done[t, i] and term_val is not None:
                c -= 1
                v_term = f(term_val[c, i]) if 0 <= c < n_slots else f(0.0)
                delta = f(f(r + f(gamma * v_term)) - v)
                run = delta
            else:
                alive = f(0.0) if done[t, i] else f(1.0)
                delta = f(f(r + f(f(gamma * next_v) * alive)) - v)
                run = f(delta + f(f(f(gamma * lam) * alive) * run))
            adv[t, i] = run
            ret[t, i] = f(run + v)
            next_v = v
    return adv, ret


def gae_boot_members(rew, val, done, last_val, term_val, term_count, gammas, lams):
    """pcc_gae_boot_pop: member m on its columns with its own gamma and lambda."""
    T, N = rew.shape
    K = len(gammas)
    n_m = N // K
    adv, ret = np.empty((T, N), dtype=np.float32), np.empty((T, N), dtype=np.float32)
    for m in range(K):
        s = slice(m * n_m, (m + 1) * n_m)
        adv[:, s], ret[:, s] = gae_boot(rew[:, s], val[:, s], done[:, s], last_val[s], None if term_val is None else term_val[:, s],
                                        None if term_count is None else term_count[s], gammas[m], lams[m])
    return adv, ret


def done_times(T, max_steps, first_done, resets=()):
    """The rows in [0, T) at which an env is done when its first done is at row first_done (0 <= first_done < max_steps) and a masked
    reset follows each row of `resets` (the step counter goes back to 0: the next done is max_steps rows later)."""
    out, steps = [], max_steps - 1 - first_done   # the counter before row 0
    for t in range(T):
        steps += 1
        if steps >= max_steps:
            out.append(t)
            steps = 0
        if t in resets:
            steps = 0
    return out
