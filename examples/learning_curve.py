#!/usr/bin/env python3
"""A learning curve that means something (GPU box): train the reference's PPO set-up on the GPU simulator for a few hundred
million env-steps, then hold the trained rate controller against baselines on envs it has never seen.

    python examples/learning_curve.py [--envs 8192] [--env-steps 2e8] [--eval-envs 4096] > profiles/r05_learning_curve.json

Training: `pcc_rl_amd.PPO` (policy shape and hyper-parameters of the reference's src/gym/stable_solve.py:30-58), whole-episode
iterations (horizon = 400 steps: every iteration averages the same mix of episode phases).  The reference trains for
6 x 1600 x 410 = 3.9e6 env-steps (stable_solve.py:54-58); the default here is ~50 times that.

Evaluation: `--eval-envs` held-out envs (another seed and another range of env ids: other links, other loss draws), one whole
400-step episode each, the SAME envs for every controller:
  trained        the trained policy's mean action (no exploration noise)
  untrained      the same network before training (mean action)
  fixed_rate     action 0 at every step: the sender stays at its starting rate, U(0.3, 1.5) x bandwidth (ns:466)
  aimd           additive increase of 1 % of the starting rate per interval, halving the rate after an interval that lost packets
                 (the textbook TCP-like rule, computed from the env's own per-step record: a baseline, not part of the library)
Reported per controller: mean episode return (the quantity PPO maximises, ns:194,205), loss ratio (lost / sent over the episode),
latency ratio (mean over steps of avg latency / connection minimum, so:183-188) and link utilisation (acknowledged packets per
second of simulated time / bandwidth).

--episode-ledger: train with PPO(track_episodes=True) -- every curve point also carries `episodes` and `true_mean_episode_return`,
the exact mean return of the episodes finished in that iteration (the key mean_episode_return stays the proxy it was: mean step
reward x episode length) -- and run the held-out evaluation through pcc_rl_amd.evaluate.evaluate: the per-episode accounting in
the library's episode ledger, one call per chunk of steps, instead of six framework additions per step."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pcc_rl_amd  # noqa: E402
from pcc_rl_amd.evaluate import evaluate as ledger_evaluate  # noqa: E402
from pcc_rl_amd.objective import parse as parse_objective  # noqa: E402
from pcc_rl_amd.ppo import PPO  # noqa: E402

COL_SENT, COL_ACKED, COL_LOST, COL_RATE, COL_TIME, COL_RUN_DUR, COL_REWARD, COL_M0 = 0, 1, 2, 3, 4, 5, 6, 7
M_LATENCY_RATIO = 10


def evaluate(name, act_fn, n, dev, seed, gid_base):
    """One whole episode of n held-out envs under act_fn(obs, env, t) -> actions [n]."""
    env = pcc_rl_amd.BatchedNetworkEnv(n, device=dev, seed=seed, env_gid_base=gid_base, record_steps=True, auto_reset=False)
    obs = env.reset()
    bw = env.state("bw")
    t0 = env.state("now").clone()
    ret = torch.zeros(n, dtype=torch.float64, device=dev)
    sent = torch.zeros(n, dtype=torch.float64, device=dev)
    acked, lost, lat_ratio = torch.zeros_like(sent), torch.zeros_like(sent), torch.zeros_like(sent)
    last = None
    for t in range(env.max_steps):
        a = act_fn(obs, env, t, last)
        obs, r, d, info = env.step(a)
        rows = info["steps"]
        last = rows
        ret += rows[:, COL_REWARD]
        sent += rows[:, COL_SENT]
        acked += rows[:, COL_ACKED]
        lost += rows[:, COL_LOST]
        lat_ratio += rows[:, COL_M0 + M_LATENCY_RATIO]
    dur = env.state("now") - t0
    env.check_flags()
    out = {"controller": name, "envs": n, "mean_episode_return": float(ret.mean()), "median_episode_return": float(ret.median()),
           "loss_ratio": float(lost.sum() / sent.sum()), "mean_latency_ratio": float((lat_ratio / env.max_steps).mean()),
           "link_utilisation": float((acked / dur / bw).mean()), "packets_per_env_step": float(sent.sum() / (n * env.max_steps))}
    env.close()
    return out


def evaluate_with_ledger(name, act_fn, n, dev, seed, gid_base):
    """evaluate() through the episode ledger: the same envs, the same keys.  The env resets itself after the episode, so the
    bandwidths are read at the first step; simulated time is the episode's total of the run_dur column."""
    env = pcc_rl_amd.BatchedNetworkEnv(n, device=dev, seed=seed, env_gid_base=gid_base)
    seen = {"t": 0, "last": None, "bw": None}

    def act(obs_row, out_row):
        if seen["bw"] is None:
            seen["bw"] = env.state("bw").clone()
        out_row.copy_(act_fn(obs_row, env, seen["t"], seen["last"]).reshape(-1))

    def hook(t, steps_row):
        seen["t"], seen["last"] = t + 1, steps_row

    r = ledger_evaluate(env, act, channels=("reward", "sent", "acked", "lost", "run_dur", "latency_ratio"), step_hook=hook)
    ret, sent, acked, dur = (r["last"][:, c] for c in (1, 2, 3, 5))
    out = {"controller": name, "envs": n, "mean_episode_return": r["channels"]["reward"]["mean"][0], "median_episode_return": float(ret.median()),
           "loss_ratio": r["loss_ratio"][0], "mean_latency_ratio": r["mean_latency_ratio"][0],
           "link_utilisation": float((acked / dur / seen["bw"]).mean()), "packets_per_env_step": float(sent.sum() / (n * env.max_steps)),
           "episodes": r["episodes"][0]}
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--env-steps", type=float, default=2e8)
    ap.add_argument("--eval-envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--normalize-obs", action="store_true",
                    help="train with PPO(normalize_obs=True); the held-out evaluation applies the trained, frozen normaliser")
    ap.add_argument("--normalize-reward", action="store_true",
                    help="train with PPO(normalize_reward=True); the curve's returns and the held-out evaluation stay raw, and every curve "
                    "point carries the value loss")
    ap.add_argument("--bootstrap-time-limit", action="store_true",
                    help="train with PPO(bootstrap_time_limit=True): the advantage estimation bootstraps from the value of the observation "
                    "an episode ended in at the step limit; every curve point carries the value loss")
    ap.add_argument("--objective", default="",
                    help="what the controller is trained for, as weights over the step records' metrics: "
                    "throughput=10,latency=-1000,loss=-2000 is the env's own reward (terms: pcc_rl_amd.objective.TERMS; a term left "
                    "out weighs 0); the rewards are recomputed on the device from the rollout's step records, 152 bytes per sample "
                    "(PPO(objective=...)); the curve's returns are then the objective's")
    ap.add_argument("--diagnostics", action="store_true",
                    help="train with PPO(diagnostics=True): every curve point carries approx_kl, clip_fraction, explained_variance and "
                    "epochs_run of that iteration's update")
    ap.add_argument("--target-kl", type=float, default=None, help="train with PPO(target_kl=...): the KL guard (implies --diagnostics)")
    ap.add_argument("--diag-rows", type=int, default=None, help="PPO(diag_rows=...): the checks read about this many of the horizon's rows")
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="train with PPO(max_grad_norm=...): every curve point carries grad_norm, max_grad_norm_seen, clipped_steps and "
                    "skipped_steps of that iteration's update")
    ap.add_argument("--rng", default="torch", choices=("torch", "philox"),
                    help="philox: the rollout's noise, the minibatch orders and the standardised advantages come from the learner's own keyed "
                    "streams on the device (PPO(rng=\"philox\")): a run does not depend on torch's generators, and the curve of --seed repeats whatever else drew from them")
    ap.add_argument("--episode-ledger", action="store_true",
                    help="train with PPO(track_episodes=True): true_mean_episode_return and episodes in every curve point, and the "
                    "held-out evaluation through pcc_rl_amd.evaluate (the library's episode ledger)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    env = pcc_rl_amd.BatchedNetworkEnv(args.envs, device=dev, seed=args.seed)
    agent = PPO(env, horizon=args.horizon, seed=args.seed, normalize_obs=args.normalize_obs, track_episodes=args.episode_ledger,
                normalize_reward=args.normalize_reward, diagnostics=args.diagnostics, target_kl=args.target_kl, diag_rows=args.diag_rows,
                max_grad_norm=args.max_grad_norm, rng=args.rng, bootstrap_time_limit=args.bootstrap_time_limit,
                objective=parse_objective(args.objective) if args.objective else None)
    untrained = {k: v.clone() for k, v in agent.policy.state_dict().items()}
    iters = max(1, int(round(args.env_steps / (args.envs * args.horizon))))
    curve = []
    t0 = time.perf_counter()
    for it in range(iters):
        s = agent.iterate()
        curve.append({"iteration": it, "env_steps": (it + 1) * args.envs * args.horizon,
                      "mean_episode_return": s["mean_step_reward"] * env.max_steps, "mean_step_reward": s["mean_step_reward"],
                      "entropy": s.get("entropy"), "value_loss": s.get("vf"), "wall_s": time.perf_counter() - t0})
        if agent.diagnostics:
            curve[-1].update({k: s[k] for k in ("approx_kl", "clip_fraction", "explained_variance", "max_log_ratio", "epochs_run")})
        if agent.grad_clip is not None:
            curve[-1].update({k: s[k] for k in ("grad_norm", "max_grad_norm_seen", "clipped_steps", "skipped_steps")})
        if args.episode_ledger:
            curve[-1].update(true_mean_episode_return=s["mean_episode_return"], episodes=s["episodes"])
    train_s = time.perf_counter() - t0
    env.check_flags()
    env.close()

    pol = agent.policy
    held = dict(n=args.eval_envs, dev=dev, seed=args.seed + 12345, gid_base=1 << 24)

    def policy_mean(obs, env_, t, last):
        with torch.no_grad():
            if args.normalize_obs:   # the trained normaliser, frozen: for the untrained network too (its inputs' scale is part of the set-up)
                obs = agent.obs_norm.normalise(obs.contiguous())
            return pol.pi(obs).reshape(-1)

    run_eval = evaluate_with_ledger if args.episode_ledger else evaluate
    results = [run_eval("trained", policy_mean, **held)]
    trained_state = {k: v.clone() for k, v in pol.state_dict().items()}
    pol.load_state_dict(untrained)
    results.append(run_eval("untrained", policy_mean, **held))
    pol.load_state_dict(trained_state)
    results.append(run_eval("fixed_rate", lambda obs, e, t, last: torch.zeros(e.n_envs, device=dev), **held))

    def aimd(obs, e, t, last):
        # rate <- rate + 1 % of the starting rate, or rate / 2 after an interval with a loss; as the env's action:
        # rate * (1 + 0.025 a) going up, rate / (1 - 0.025 a) going down (ns:235-241)
        rate = e.state("rate")[0]
        rate0 = e.state("rate0")[0]
        up = (0.01 * rate0 / rate) / 0.025
        down = torch.full_like(up, -40.0)               # rate / (1 + 1)
        if last is None:
            return up.to(torch.float32)
        return torch.where(last[:, COL_LOST] > 0, down, up).to(torch.float32)

    results.append(run_eval("aimd", aimd, **held))
    by = {r["controller"]: r for r in results}
    out = {"what": "PPO (reference hyper-parameters, pi/vf MLP 32-16) on the MI355X simulator, then the trained controller against "
                   "baselines on held-out envs; python examples/learning_curve.py",
           "normalize_obs": bool(args.normalize_obs), "normalize_reward": bool(args.normalize_reward),
           "bootstrap_time_limit": bool(args.bootstrap_time_limit), "objective": args.objective or None, "episode_ledger": bool(args.episode_ledger),
           "diagnostics": bool(agent.diagnostics), "target_kl": args.target_kl, "diag_rows": args.diag_rows, "max_grad_norm": args.max_grad_norm,
           "training": {"envs": args.envs, "horizon": args.horizon, "iterations": iters, "env_steps": iters * args.envs * args.horizon,
                        "reference_budget_env_steps": 6 * 1600 * 410, "wall_s": train_s,
                        "env_steps_per_s_incl_learning": iters * args.envs * args.horizon / train_s,
                        "first_iteration_return": curve[0]["mean_episode_return"], "last_iteration_return": curve[-1]["mean_episode_return"],
                        "best_iteration_return": max(c["mean_episode_return"] for c in curve)},
           "held_out_evaluation": results,
           "trained_vs": {k: {"return_gain": by["trained"]["mean_episode_return"] - by[k]["mean_episode_return"]}
                          for k in ("untrained", "fixed_rate", "aimd")},
           "curve": curve}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
