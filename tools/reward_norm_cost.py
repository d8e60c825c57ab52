#!/usr/bin/env python3
"""What reward normalisation costs (GPU box only), two things in one process --
  (a) kernels      the library's calls alone on one rollout's [horizon][envs] reward and done rows: RewardNormalizer.update (the walk
                   and the merge, two launches) + normalise (one launch), for every --members count at every --envs size, next to the
                   same accounting in torch: a loop over the steps with `where` on done, then a per-member `var` of the samples
  (b) iterate      PPO.iterate() and PopulationPPO.iterate() (K = --population) at --iterate-envs x --horizon, without and with
                   normalize_reward (--no-iterate leaves it out)
The variants of each group alternate, --repeats repeats after a warm-up of each, a host clock around a device synchronise.
Microseconds per call, min - max over the repeats.  The walk reads 4 + 1 bytes per sample and 8 + 8 bytes of carry per env; the
normalise reads and writes 4 bytes per sample: the achieved bytes per second are those over the time of the minimum.
   python tools/reward_norm_cost.py [--out profiles/r23_reward_norm.json] [--envs 65536,262144] [--horizon 64] [--members 1,8,32]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r23_reward_norm.json"))
ap.add_argument("--envs", default="65536,262144")
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--members", default="1,8,32")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--inner", type=int, default=50, help="calls per timed window of (a)")
ap.add_argument("--torch-inner", type=int, default=5, help="calls per timed window of the torch restatement of (a)")
ap.add_argument("--iterate-envs", type=int, default=65536)
ap.add_argument("--population", type=int, default=4)
ap.add_argument("--iterate-inner", type=int, default=2, help="iterate() calls per timed window of (b)")
ap.add_argument("--no-iterate", action="store_true")
args = ap.parse_args()

import torch
import pcc_rl_amd
from pcc_rl_amd import build as pbuild
from pcc_rl_amd.ppo import PPO, PopulationPPO
from pcc_rl_amd.rewnorm import RewardNormalizer

dev = torch.device("cuda:0")


def timed(fn, inner):
    """microseconds per call over a window of `inner` consecutive calls"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e6


def alternate(variants):
    """{name: [us per repeat]} of {name: (fn, inner)}: a warm-up window of every variant, then --repeats rounds, the variants alternating"""
    times = {name: [] for name in variants}
    for rep in range(-1, args.repeats):
        for name, (fn, inner) in variants.items():
            t = timed(fn, inner)
            if rep >= 0:
                times[name].append(t)
    return times


def summary(times):
    out = {}
    for name, t in times.items():
        out[name + "_us"] = t
        out[name + "_us_min_max"] = [min(t), max(t)]
    return out


T = args.horizon
out = {"what": "microseconds per call, host clock around a device synchronise, the variants of a group alternating, %d repeats after a warm-up "
               "of each: (a) RewardNormalizer.update / normalise on [%d][envs] rows, windows of %d calls, and the same accounting in torch, "
               "windows of %d calls; (b) iterate() without and with normalize_reward, windows of %d calls"
               % (args.repeats, T, args.inner, args.torch_inner, args.iterate_inner),
       "device": torch.cuda.get_device_name(0), "build": pbuild.build_info(), "repeats": args.repeats, "horizon": T}

# (a) ---------------------------------------------------------------------------------------------------------------------
g = torch.Generator(device=dev).manual_seed(1)
for N in [int(x) for x in args.envs.split(",")]:
    rew_b = torch.randn((T, N), device=dev, generator=g) * 3.0 - 1.0
    done_b = torch.rand((T, N), device=dev, generator=g) < 0.05
    rew_out = torch.empty_like(rew_b)
    for members in [int(x) for x in args.members.split(",")]:
        nz = RewardNormalizer(N, members, device=dev)
        hyper = torch.zeros((members, 8), device=dev)
        hyper[:, 3] = torch.linspace(0.9, 0.99, members, device=dev)
        n_m = N // members
        t_carry = torch.zeros(N, dtype=torch.float64, device=dev)
        t_stats = torch.zeros((members, 3), dtype=torch.float64, device=dev)
        gam = hyper[:, 3].double().repeat_interleave(n_m)

        def torch_update():
            R = t_carry
            samples = torch.empty((T, N), dtype=torch.float64, device=dev)
            for t in range(T):
                R = R * gam + rew_b[t]
                samples[t] = R
                R = torch.where(done_b[t], torch.zeros_like(R), R)
            t_carry.copy_(R)
            var, mean = torch.var_mean(samples.view(T, members, n_m), dim=(0, 2), unbiased=False)
            nb = float(T * n_m)
            na, ma, qa = t_stats[:, 0].clone(), t_stats[:, 1].clone(), t_stats[:, 2].clone()
            n = na + nb
            d = mean - ma
            t_stats[:, 1] = ma + d * nb / n
            t_stats[:, 2] = qa + var * nb + d * d * na * nb / n
            t_stats[:, 0] = n
            scale = (1.0 / torch.sqrt(t_stats[:, 2] / n + 1e-8)).float()
            return torch.clamp(rew_b.view(T, members, n_m) * scale[None, :, None], -10.0, 10.0)

        # one call of each from the empty state: the torch restatement and the library count the same samples and agree
        nz.update(rew_b, done_b, hyper)
        torch_update()
        rel = ((t_stats[:, 2] / t_stats[:, 0]) / (nz.stats[:, 2] / nz.stats[:, 0]) - 1.0).abs().max()
        same = bool(torch.equal(t_stats[:, 0], nz.stats[:, 0]) and torch.equal(t_carry, nz.ret_carry))
        times = alternate({"kernel_update": (lambda: nz.update(rew_b, done_b, hyper), args.inner),
                           "kernel_normalise": (lambda: nz.normalise(rew_b, rew_out), args.inner),
                           "kernel_update_and_normalise": (lambda: (nz.update(rew_b, done_b, hyper), nz.normalise(rew_b, rew_out)), args.inner),
                           "torch_update_and_normalise": (torch_update, args.torch_inner)})
        row = summary(times)
        row["torch_variance_relative_difference_after_one_call"] = float(rel)
        row["torch_count_and_carry_equal_after_one_call"] = same
        row["update_bytes"] = T * N * 5 + N * 16
        row["normalise_bytes"] = T * N * 8
        row["kernel_update_gb_per_s_of_min"] = row["update_bytes"] / (min(times["kernel_update"]) * 1e-6) / 1e9
        row["kernel_normalise_gb_per_s_of_min"] = row["normalise_bytes"] / (min(times["kernel_normalise"]) * 1e-6) / 1e9
        out["calls_envs_%d_members_%d" % (N, members)] = row
        print("envs = %d, members = %d: %s" % (N, members, json.dumps(row)), flush=True)
        del nz
    del rew_b, done_b, rew_out
    torch.cuda.empty_cache()

# (b) ---------------------------------------------------------------------------------------------------------------------
# The env's step time depends on what the policy does (packets in flight), and a policy trained on other rewards does something else:
# the "frozen" pair runs with lr = 0 -- the same launches, the policies stay what they were -- so that the two trainers step the
# same kind of trajectories and the difference is the option's own work.
if not args.no_iterate:
    N, K = args.iterate_envs, args.population
    for name, make in (("ppo", lambda env, on: PPO(env, horizon=T, seed=0, minibatch=max(2048, N * T // 4), normalize_reward=on)),
                       ("ppo_frozen", lambda env, on: PPO(env, horizon=T, seed=0, minibatch=max(2048, N * T // 4), lr=0.0, normalize_reward=on)),
                       ("population_k%d" % K, lambda env, on: PopulationPPO(env, K, horizon=T, normalize_reward=on)),
                       ("population_k%d_frozen" % K, lambda env, on: PopulationPPO(env, K, horizon=T, lr=0.0, normalize_reward=on))):
        envs = [pcc_rl_amd.BatchedNetworkEnv(N, device=dev, seed=0, ring_pools=(1, 2, 8)) for _ in range(2)]
        plain, normed = make(envs[0], False), make(envs[1], True)
        times = alternate({"iterate_plain": (plain.iterate, args.iterate_inner), "iterate_normalised": (normed.iterate, args.iterate_inner)})
        for e in envs:
            e.check_flags()
            e.close()
        row = summary(times)
        row["added_us_of_min"] = min(times["iterate_normalised"]) - min(times["iterate_plain"])
        out["iterate_" + name] = row
        print("%s: %s" % (name, json.dumps(row)), flush=True)
        del plain, normed, envs
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
