#!/usr/bin/env python3
"""Train a PCC rate controller with PPO on the GPU simulator.

    python examples/train_ppo.py --envs 8192 --iters 50 [--arch=32,16] [--gamma=0.99]
    python examples/train_ppo.py --iters 50 --checkpoint run.pt --checkpoint-every 10     # ... interrupted ...
    python examples/train_ppo.py --iters 50 --resume run.pt --checkpoint run.pt           # goes on where run.pt was written, bit for bit

Counterpart of the reference's src/gym/stable_solve.py, but with the env, the rollout buffers and
the optimiser all on one MI355X (see pcc-rl_amd/ppo.py)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pcc_rl_amd  # noqa: E402
from pcc_rl_amd.objective import parse as parse_objective  # noqa: E402
from pcc_rl_amd.ppo import PPO  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--arch", default="32,16")
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--save", default="")
    ap.add_argument("--normalize-obs", action="store_true",
                    help="standardise the observations with running moments on the device (PPO(normalize_obs=True)); the normaliser "
                    "travels in --checkpoint / --resume, in --save and in --export")
    ap.add_argument("--normalize-reward", action="store_true",
                    help="divide the rewards the advantage estimation reads by the running standard deviation of the discounted return, on the "
                    "device (PPO(normalize_reward=True)); the statistics travel in --checkpoint / --resume; what is printed stays raw")
    ap.add_argument("--bootstrap-time-limit", action="store_true",
                    help="every done of this env is the step limit, not a terminal state: bootstrap the advantage estimation from the "
                    "value of the observation the episode ended in, rebuilt on the device (PPO(bootstrap_time_limit=True)); holds the "
                    "step records of a rollout, 152 bytes per sample")
    ap.add_argument("--objective", default="",
                    help="what the controller is trained for, as weights over the step records' metrics: "
                    "throughput=10,latency=-1000,loss=-2000 is the env's own reward (terms: pcc_rl_amd.objective.TERMS; a term left "
                    "out weighs 0); the rewards are recomputed on the device from the rollout's step records, 152 bytes per sample "
                    "(PPO(objective=...))")
    ap.add_argument("--diagnostics", action="store_true",
                    help="after every epoch of an update compute the approximate KL divergence from the rollout's policy, the clip fraction over "
                    "the whole rollout and the explained variance of the value function on the device (PPO(diagnostics=True))")
    ap.add_argument("--target-kl", type=float, default=None,
                    help="stop updating the policy for the rest of an update once its approximate KL exceeds 1.5 x this after an epoch, decided on "
                    "the device (implies --diagnostics)")
    ap.add_argument("--diag-rows", type=int, default=None, help="the checks read about this many of the horizon's rows (default: all)")
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="limit the global norm of every optimiser step's gradient to this, and leave out a step whose gradient is not finite, "
                    "on the device (PPO(max_grad_norm=...); 0: that guard alone; stable-baselines3's default is 0.5)")
    ap.add_argument("--rng", default="torch", choices=("torch", "philox"),
                    help="philox: the rollout's noise, the minibatch orders and the standardised advantages come from the learner's own keyed "
                    "streams on the device (PPO(rng=\"philox\")): a run does not depend on torch's generators, and equals the member with the same seed of any population on the same env ids")
    ap.add_argument("--export", default="", help="write the trained policy here as TorchScript (export.export_policy)")
    ap.add_argument("--policy-in-step", action="store_true",
                    help="collect each horizon as one closed-loop call (pcc_rollout): the policy inside the env's launches")
    ap.add_argument("--checkpoint", default="", help="write the whole training state here (PPO.state_dict: policy, Adam, generators, "
                    "the env's snapshot) every --checkpoint-every iterations and at the end")
    ap.add_argument("--checkpoint-every", type=int, default=10)
    ap.add_argument("--resume", default="", help="continue from a --checkpoint file of a run with the same --envs, --horizon and --arch")
    ap.add_argument("--ring-pools", default="", help="div1,div2,div3 of BatchedNetworkEnv(ring_pools=...); with --checkpoint / --resume the "
                    "default is 2,8,32 (the library's own default depends on the free device memory, and a snapshot needs equal pools)")
    args = ap.parse_args()
    pools = tuple(int(x) for x in args.ring_pools.split(",")) if args.ring_pools else ((2, 8, 32) if args.checkpoint or args.resume else None)
    env = pcc_rl_amd.BatchedNetworkEnv(args.envs, device="cuda:0", seed=0, ring_pools=pools)
    agent = PPO(env, arch=tuple(int(x) for x in args.arch.split(",")), gamma=args.gamma, horizon=args.horizon,
                policy_in_step=args.policy_in_step, normalize_obs=args.normalize_obs, normalize_reward=args.normalize_reward,
                diagnostics=args.diagnostics, target_kl=args.target_kl, diag_rows=args.diag_rows, max_grad_norm=args.max_grad_norm,
                rng=args.rng, bootstrap_time_limit=args.bootstrap_time_limit,
                objective=parse_objective(args.objective) if args.objective else None)
    first = 0
    if args.resume:
        ck = torch.load(args.resume)
        agent.load_state_dict(ck["ppo"])
        first = int(ck["iters_done"])
        print("resumed %s after %d iterations" % (args.resume, first))

    def checkpoint(done):
        torch.save({"ppo": agent.state_dict(), "iters_done": done}, args.checkpoint + ".tmp")
        os.replace(args.checkpoint + ".tmp", args.checkpoint)

    t0 = time.perf_counter()
    for it in range(first, args.iters):
        s = agent.iterate()
        if args.checkpoint and ((it + 1) % max(args.checkpoint_every, 1) == 0 or it + 1 == args.iters):
            checkpoint(it + 1)
        steps = (it + 1 - first) * args.envs * args.horizon
        diag = ("  kl %.4f  clipped %.3f  explained variance %6.3f  epochs %d"
                % (s["approx_kl"], s["clip_fraction"], s["explained_variance"], s["epochs_run"])) if agent.diagnostics else ""
        if agent.grad_clip is not None:
            diag += "  grad norm %.3f (max %.3f)  clipped %d  skipped %d" % (s["grad_norm"], s["max_grad_norm_seen"], s["clipped_steps"],
                                                                          s["skipped_steps"])
        print("iter %3d  env-steps %10d  reward/step %8.4f  entropy %6.3f  %.0f env-steps/s incl. learning%s"
              % (it, steps, s["mean_step_reward"], s["entropy"], steps / (time.perf_counter() - t0), diag))
    obs_norm = agent.obs_norm.member(0) if args.normalize_obs else None   # (shift, scale, clip): the policy is meaningless without it
    if args.save:
        torch.save({"policy": agent.policy.state_dict(), "obs_norm": obs_norm} if args.normalize_obs else agent.policy.state_dict(), args.save)
    if args.export:
        from pcc_rl_amd.export import export_policy
        export_policy(agent.policy, args.export, obs_norm=obs_norm)


if __name__ == "__main__":
    main()
