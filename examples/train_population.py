#!/usr/bin/env python3
"""Train a population of PCC rate controllers -- K independent PPO learners on K slices of one env batch (pcc-rl_amd/ppo.py:
PopulationPPO): seeds for a learning curve, or a sweep over learning rates, entropy coefficients and discount factors.

    python examples/train_population.py --members 8 --envs 65536 --iters 50                  # eight seeds
    python examples/train_population.py --members 4 --envs 32768 --lrs 1e-3,3e-4,1e-4,3e-5   # a learning-rate sweep
    python examples/train_population.py --members 4 --envs 32768 --checkpoint pop.pt         # ... interrupted ... (--ring-pools 1,2,8 at 65 536 envs)
    python examples/train_population.py --members 4 --envs 32768 --resume pop.pt --checkpoint pop.pt
    python examples/train_population.py --members 8 --lrs 1e-2,3e-3,1e-3,3e-4,1e-4,3e-5,1e-5,3e-6 --pbt-every 5   # population-based training

One line per iteration with every member's episode return.  --lrs / --ent-coefs / --gammas take one value or one per member.
--pbt-every N: every N iterations the worst --pbt-frac of the members take over a good member's weights, Adam state and
hyper-parameters, lr and ent_coef perturbed (PopulationPPO.evolve: one launch, scored by the mean reward over those N iterations);
the line then also shows every member's parent, lr and ent_coef.  The generation travels in --checkpoint / --resume.
--pbt-score episode_return: the generations are scored by the mean return of the episodes each member finished since the last
one, counted exactly on the device (PopulationPPO(track_episodes=True): evolve() reads the episode ledger itself), and the line
also shows every member's episodes and true mean episode return of the iteration."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pcc_rl_amd  # noqa: E402
from pcc_rl_amd.env import MAX_STEPS  # noqa: E402
from pcc_rl_amd.objective import parse as parse_objective  # noqa: E402
from pcc_rl_amd.ppo import PopulationPPO  # noqa: E402


def values(text, default):
    """one value for all members, or one per member (PopulationPPO checks the count)"""
    if not text:
        return default
    v = [float(x) for x in text.split(",")]
    return v[0] if len(v) == 1 else v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--envs", type=int, default=65536, help="of the whole batch: every member trains on envs / members of them")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--arch", default="32,16")
    ap.add_argument("--lrs", default="")
    ap.add_argument("--ent-coefs", default="")
    ap.add_argument("--gammas", default="")
    ap.add_argument("--seeds", default="", help="one per member (default 0, 1, ...)")
    ap.add_argument("--save", default="", help="write every member's policy state_dict here (a list) at the end")
    ap.add_argument("--normalize-obs", action="store_true",
                    help="every member standardises its observations with its own running moments on the device "
                    "(PopulationPPO(normalize_obs=True)); the normalisers travel in --checkpoint / --resume, --save and --export, and "
                    "with the weights in a --pbt-every generation")
    ap.add_argument("--normalize-reward", action="store_true",
                    help="every member divides the rewards its advantage estimation reads by the running standard deviation of its own "
                    "discounted return, with its own gamma (PopulationPPO(normalize_reward=True)); the statistics travel in --checkpoint / "
                    "--resume and with the weights in a --pbt-every generation; scores and what is printed stay raw")
    ap.add_argument("--bootstrap-time-limit", action="store_true",
                    help="every done of this env is the step limit, not a terminal state: every member bootstraps its advantage estimation "
                    "from its own value of the observation the episode ended in, rebuilt on the device "
                    "(PopulationPPO(bootstrap_time_limit=True)); holds the step records of a rollout, 152 bytes per sample")
    ap.add_argument("--objective", default="",
                    help="what the controller is trained for, as weights over the step records' metrics: "
                    "throughput=10,latency=-1000,loss=-2000 is the env's own reward (terms: pcc_rl_amd.objective.TERMS; a term left "
                    "out weighs 0); the rewards are recomputed on the device from the rollout's step records, 152 bytes per sample "
                    "(PopulationPPO(objective=...)); with ';' between members one objective per member, one entry applies to all; the weights stay with their slots in a --pbt-every generation, and --pbt-score episode_return needs one objective for all")
    ap.add_argument("--diagnostics", action="store_true",
                    help="after every epoch of an update compute the approximate KL divergence from the rollout's policy, the clip fraction over "
                    "the whole rollout and the explained variance of the value function on the device (PopulationPPO(diagnostics=True))")
    ap.add_argument("--target-kl", type=float, default=None,
                    help="stop updating a member for the rest of an update once its approximate KL exceeds 1.5 x this after an epoch, decided on "
                    "the device (implies --diagnostics)")
    ap.add_argument("--diag-rows", type=int, default=None, help="the checks read about this many of the horizon's rows (default: all)")
    ap.add_argument("--max-grad-norm", default="",
                    help="one limit, or one per member (comma-separated), on the global norm of every optimiser step's gradient; a member's "
                    "step whose gradient is not finite is left out (PopulationPPO(max_grad_norm=...); 0: that guard alone).  The limit is a "
                    "column of the hyper block: a replaced member takes its parent's in a --pbt-every generation")
    ap.add_argument("--rng", default="torch", choices=("torch", "philox"),
                    help="philox: the rollout's noise, the minibatch orders and the standardised advantages come from every member's own keyed "
                    "streams on the device (PopulationPPO(rng=\"philox\")): a run does not depend on torch's generators, and a member repeats when it is run alone with its seed, in a population of another size or in another slot")
    ap.add_argument("--export", default="", help="write every member's policy as TorchScript into <dir>/member<m> (export.export_policy)")
    ap.add_argument("--checkpoint", default="", help="write the whole training state here every --checkpoint-every iterations and at the end")
    ap.add_argument("--checkpoint-every", type=int, default=10)
    ap.add_argument("--resume", default="", help="continue from a --checkpoint file of a run with the same --members, --envs, --horizon and --arch")
    ap.add_argument("--pbt-every", type=int, default=0, help="evolve the population every N iterations (0: never, a static sweep)")
    ap.add_argument("--pbt-frac", type=float, default=0.25, help="the share of the members replaced per generation (at most 0.5)")
    ap.add_argument("--pbt-seed", type=int, default=0)
    ap.add_argument("--pbt-score", default="step_reward", choices=("step_reward", "episode_return"),
                    help="what a generation selects on: the mean step reward of its iterations (default), or the mean return of the "
                    "episodes finished in them (the episode ledger; needs --pbt-every x --horizon >= the episode length)")
    ap.add_argument("--curve", default="", help="write every iteration's returns per member -- and each generation's parents and hyper rows -- here as JSON")
    ap.add_argument("--ring-pools", default="", help="div1,div2,div3 of BatchedNetworkEnv(ring_pools=...); with --checkpoint / --resume the "
                    "default is 2,8,32 (the library's own default depends on the free device memory, and a snapshot needs equal pools): "
                    "untrained policies ran those dry at 65 536 envs (PCC_FLAG_POOL_EXHAUSTED) -- 1,2,8 held there; the same on the run that resumes")
    args = ap.parse_args()
    pools = tuple(int(x) for x in args.ring_pools.split(",")) if args.ring_pools else ((2, 8, 32) if args.checkpoint or args.resume else None)
    ledger = args.pbt_score == "episode_return"
    if ledger and args.pbt_every * args.horizon < MAX_STEPS:   # (said before a device is touched)
        ap.error("--pbt-score episode_return: a generation of --pbt-every x --horizon = %d steps is shorter than an episode (%d steps): "
                 "no member would finish one" % (args.pbt_every * args.horizon, MAX_STEPS))
    env = pcc_rl_amd.BatchedNetworkEnv(args.envs, device="cuda:0", seed=0, ring_pools=pools)
    pop = PopulationPPO(env, args.members, arch=tuple(int(x) for x in args.arch.split(",")), horizon=args.horizon,
                        lr=values(args.lrs, 1e-3), ent_coef=values(args.ent_coefs, 0.01),
                        gamma=values(args.gammas, 0.99),
                        seeds=[int(x) for x in args.seeds.split(",")] if args.seeds else None, normalize_obs=args.normalize_obs,
                        track_episodes=ledger, normalize_reward=args.normalize_reward,
                        diagnostics=args.diagnostics, target_kl=args.target_kl, diag_rows=args.diag_rows,
                        max_grad_norm=values(args.max_grad_norm, None) if args.max_grad_norm else None, rng=args.rng,
                        bootstrap_time_limit=args.bootstrap_time_limit,
                        objective=parse_objective(args.objective) if args.objective else None)
    first = 0
    if args.resume:
        ck = torch.load(args.resume)
        pop.load_state_dict(ck["population"])
        first = int(ck["iters_done"])
        print("resumed %s after %d iterations" % (args.resume, first))

    window = []   # the members' mean step rewards of the iterations since the last generation
    if args.resume and args.pbt_every > 0:
        window = [list(r) for r in ck.get("pbt_window", [])]

    def checkpoint(done):
        torch.save({"population": pop.state_dict(), "iters_done": done, "pbt_window": window}, args.checkpoint + ".tmp")
        os.replace(args.checkpoint + ".tmp", args.checkpoint)

    curve = {"args": vars(args), "returns": [], "generations": []}
    t0 = time.perf_counter()
    for it in range(first, args.iters):
        s = pop.iterate()
        curve["returns"].append([r * env.max_steps for r in s["mean_step_reward"]])
        pbt = ""
        if args.pbt_every > 0:
            window.append(s["mean_step_reward"])
            if len(window) >= args.pbt_every:
                scores = None if ledger else torch.tensor(window, dtype=torch.float64).mean(dim=0)   # (None: the ledger's, on the device)
                parent, _ = pop.evolve(scores, frac=args.pbt_frac, seed=args.pbt_seed)
                window = []
                curve["generations"].append({"after_iter": it, "parents": parent.tolist(), "hyper": pop.hypers()})
                pbt = "  parents: %s  lr: %s  ent_coef: %s" % (" ".join("%d" % p for p in parent.tolist()),
                                                             " ".join("%.2e" % h[0] for h in pop.hypers()), " ".join("%.2e" % h[2] for h in pop.hypers()))
        if args.checkpoint and ((it + 1) % max(args.checkpoint_every, 1) == 0 or it + 1 == args.iters):
            checkpoint(it + 1)
        if ledger:
            curve.setdefault("episodes", []).append(s["episodes"])
            curve.setdefault("true_mean_episode_return", []).append(s["mean_episode_return"])
            pbt = "  episodes: %s  true return: %s%s" % (" ".join("%d" % e for e in s["episodes"]),
                                                          " ".join("%7.1f" % r for r in s["mean_episode_return"]), pbt)
        if pop.grad_clip is not None:
            for key in ("grad_norm", "max_grad_norm_seen", "clipped_steps", "skipped_steps"):
                curve.setdefault(key, []).append(s[key])
            pbt = "  grad norm: %s  clipped: %s  skipped: %s%s" % (" ".join("%.3f" % g for g in s["grad_norm"]),
                                                                   " ".join("%d" % n for n in s["clipped_steps"]),
                                                                   " ".join("%d" % n for n in s["skipped_steps"]), pbt)
        if pop.diagnostics:
            for key in ("approx_kl", "clip_fraction", "explained_variance", "epochs_run"):
                curve.setdefault(key, []).append(s[key])
            pbt = "  kl: %s  epochs: %s%s" % (" ".join("%.4f" % k for k in s["approx_kl"]), " ".join("%d" % e for e in s["epochs_run"]), pbt)
        steps = (it + 1 - first) * args.envs * args.horizon
        print("iter %3d  env-steps %11d  %.0f env-steps/s incl. learning  return per member: %s%s"
              % (it, steps, steps / (time.perf_counter() - t0), " ".join("%7.1f" % (r * env.max_steps) for r in s["mean_step_reward"]), pbt))
    if args.curve:
        import json
        curve["hyper_at_end"] = pop.hypers()
        with open(args.curve, "w") as f:
            json.dump(curve, f, indent=1)
    norms = [pop.obs_norm.member(m) for m in range(args.members)] if args.normalize_obs else None   # (shift, scale, clip) per member
    if args.save:
        states = [p.state_dict() for p in pop.policies]
        torch.save({"policies": states, "obs_norm": norms} if args.normalize_obs else states, args.save)
    if args.export:
        from pcc_rl_amd.export import export_policy
        for m, p in enumerate(pop.policies):
            export_policy(p, os.path.join(args.export, "member%d" % m), obs_norm=norms[m] if norms else None)


if __name__ == "__main__":
    main()
