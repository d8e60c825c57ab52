"""Held-out evaluation through the episode ledger (episodes.EpisodeLedger): whole episodes of an env batch
under any controller, the per-episode accounting in one library call per chunk of steps instead of framework additions per
step, nothing read back until the end."""
import torch

from .episodes import EpisodeLedger, summarise
from .native import PCC_STEP_COLS
from .objective import RewardObjective

STEPS_BYTES = 256 << 20   # the step-record buffer of a chunk stays under this


def evaluate(env, act, episodes=1, channels=("sent", "acked", "lost", "run_dur", "latency_ratio"), members=1, step_hook=None,
             objective=None):
    """Reset `env` (a BatchedNetworkEnv with one sender and auto_reset) and step it episodes * env.max_steps times, every env
    `episodes` whole episodes.  act(obs_row, out_act_row) writes the actions [N] for the observation row [N, D] into
    out_act_row -- a trained policy's mean through pcc_policy_act(_pop) with noise=None, or a baseline; step_hook(t, steps_row),
    if given, sees the step-record row [N, 19] step t just wrote (a device tensor: a baseline that needs the last interval's
    counters).  Each chunk's reward, done and step-record rows go into an EpisodeLedger with `channels` over `members` slices.
    Returns the ledger's summary() plus, per member, loss_ratio = sum(lost) / sum(sent) and mean_latency_ratio = sum(latency
    ratio) / steps where the channels are there, and the per-env tensors last / last_len of the last finished episodes (device).
    objective: an objective.RewardObjective over the env batch, or what makes one for `members` members: the
    ledger's channel 0 is fed the objective's rows of each chunk's step records instead of the env's reward rows; add "reward" to
    `channels` for the env's own returns beside them."""
    if env.n_senders != 1:
        raise ValueError("evaluate: one sender per env (n_senders = %d): the ledger's rows are [T][n_envs]" % env.n_senders)
    if not env.auto_reset:
        raise ValueError("evaluate: the env must reset itself at an episode's end (auto_reset=True)")
    episodes = int(episodes)
    if episodes < 1:
        raise ValueError("evaluate: episodes = %d (>= 1)" % episodes)
    N, D, dev = env.n_envs, env.obs_dim, env.device
    ledger = EpisodeLedger(N, members, channels, device=dev)
    if objective is not None and not isinstance(objective, RewardObjective):
        objective = RewardObjective(N, members, objective, device=dev)
    if objective is not None and objective.n_envs != N:
        raise ValueError("evaluate: a RewardObjective of %d envs for an env batch of %d" % (objective.n_envs, N))
    total = episodes * env.max_steps
    chunk = max(1, min(total, (STEPS_BYTES - 1) // (N * PCC_STEP_COLS * 8)))
    obs = torch.empty((chunk + 1, N, D), device=dev)
    act_b = torch.empty((chunk, N), device=dev)
    rew = torch.empty((chunk, N), device=dev)
    done = torch.empty((chunk, N), dtype=torch.uint8, device=dev)
    steps = torch.empty((chunk, N, PCC_STEP_COLS), dtype=torch.float64, device=dev)
    obs[0] = env.reset()
    t = 0
    while t < total:
        n = min(chunk, total - t)
        for k in range(n):
            act(obs[k], act_b[k])
            env.step_many(act_b[k:k + 1], obs_out=obs[k + 1:k + 2], reward_out=rew[k:k + 1], done_out=done[k:k + 1],
                          steps_out=steps[k:k + 1])
            if step_hook is not None:
                step_hook(t + k, steps[k])
        ledger.update(rew[:n] if objective is None else objective.apply(steps[:n]), done[:n], steps[:n])
        obs[0] = obs[n]
        t += n
    env.check_flags()
    rows = ledger.totals().tolist()   # the one read-back
    out = summarise(rows, ledger.names)
    nan = float("nan")

    def total_of(name):
        c = ledger.names.index(name)
        return [r[2 + 4 * c] for r in rows]
    if "sent" in ledger.names and "lost" in ledger.names:
        out["loss_ratio"] = [lo / s if s > 0 else nan for lo, s in zip(total_of("lost"), total_of("sent"))]
    if "latency ratio" in ledger.names:
        out["mean_latency_ratio"] = [x / r[1] if r[1] > 0 else nan for x, r in zip(total_of("latency ratio"), rows)]
    out["last"], out["last_len"] = ledger.last, ledger.last_len
    return out
