#!/usr/bin/env python3
"""What observation normalisation costs (GPU box only), three things in one process --
  (a) collect      PPO.collect() and PopulationPPO.collect() (K = --members) at --envs x --horizon, with and without normalize_obs: the
                   comparison is the un-normalised collect() of the same run
  (b) kernels      the library's calls alone: pcc_obs_stats_update_pop on one rollout's [horizon][envs][D] rows (two launches) and
                   pcc_obs_normalise_pop on one [envs][D] row block (one launch), for 1 and K members
  (c) framework    the same work in torch: clamp((x - m) * s) per step, and per rollout a per-member loop of var_mean (float32, as a
                   user would write it) with Chan's merge into running rows
The variants of each group alternate, --repeats repeats after a warm-up of each, a host clock around a device synchronise.
Microseconds per call, min - max over the repeats.
   python tools/obs_norm_cost.py [--out profiles/r16_obs_norm.json] [--envs 65536] [--horizon 64] [--members 8]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r16_obs_norm.json"))
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--members", type=int, default=8)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--inner", type=int, default=50, help="calls per timed window of (b) and (c)")
ap.add_argument("--collect-inner", type=int, default=2, help="collect() calls per timed window of (a)")
args = ap.parse_args()

import torch
import pcc_rl_amd
from pcc_rl_amd import build as pbuild
from pcc_rl_amd.obsnorm import ObsNormalizer
from pcc_rl_amd.ppo import PPO, PopulationPPO

dev = torch.device("cuda:0")


def timed(fn, inner):
    """microseconds per call over a window of `inner` consecutive calls"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e6


def alternate(variants, inner):
    """{name: [us per repeat]}: a warm-up window of every variant, then --repeats rounds, the variants alternating"""
    times = {name: [] for name in variants}
    for rep in range(-1, args.repeats):
        for name, fn in variants.items():
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


T, N, K = args.horizon, args.envs, args.members
out = {"what": "microseconds per call, host clock around a device synchronise, the variants of a group alternating, %d repeats after a warm-up "
               "of each: (a) collect() of %d envs x %d steps with and without normalize_obs, windows of %d calls; (b) the library's calls alone and "
               "(c) the same work in torch, windows of %d calls" % (args.repeats, N, T, args.collect_inner, args.inner),
       "device": torch.cuda.get_device_name(0), "build": pbuild.build_info(), "repeats": args.repeats, "n_envs": N, "horizon": T, "members": K}

# (a) ---------------------------------------------------------------------------------------------------------------------
for name, make in (("ppo", lambda env, on: PPO(env, horizon=T, normalize_obs=on)),
                   ("population_k%d" % K, lambda env, on: PopulationPPO(env, K, horizon=T, normalize_obs=on))):
    envs = [pcc_rl_amd.BatchedNetworkEnv(N, device=dev, seed=0, ring_pools=(1, 2, 8)) for _ in range(2)]
    plain, normed = make(envs[0], False), make(envs[1], True)
    times = alternate({"collect_plain": plain.collect, "collect_normalised": normed.collect}, args.collect_inner)
    for e in envs:
        e.check_flags()
        e.close()
    row = summary(times)
    row["added_us_of_min"] = min(times["collect_normalised"]) - min(times["collect_plain"])
    row["added_fraction_of_min"] = row["added_us_of_min"] / min(times["collect_plain"])
    out["collect_" + name] = row
    print("%s: %s" % (name, json.dumps(row)), flush=True)
    del plain, normed, envs
    torch.cuda.empty_cache()

# (b), (c) ----------------------------------------------------------------------------------------------------------------
D = 30
g = torch.Generator(device=dev).manual_seed(1)
raw_b = torch.randn((T, N, D), device=dev, generator=g) * 50.0 + 20.0
row_out = torch.empty((N, D), device=dev)
for members in sorted({1, K}):
    nz = ObsNormalizer(D, members, device=dev)
    nz.update(raw_b)
    n_m = N // members
    t_stats = torch.zeros((members, 1 + 2 * D), dtype=torch.float64, device=dev)

    def torch_normalise():
        shift, scale = nz.norm[:, None, :D], nz.norm[:, None, D:]
        return torch.clamp((raw_b[0].view(members, n_m, D) - shift) * scale, -nz.clip, nz.clip)

    def torch_update():
        for m in range(members):
            var, mean = torch.var_mean(raw_b[:, m * n_m:(m + 1) * n_m], dim=(0, 1), unbiased=False)
            nb = float(T * n_m)
            na, ma, qa = t_stats[m, 0], t_stats[m, 1:1 + D], t_stats[m, 1 + D:]
            n = na + nb
            d = mean.double() - ma
            t_stats[m, 1:1 + D] = ma + d * nb / n
            t_stats[m, 1 + D:] = qa + var.double() * nb + d * d * na * nb / n
            t_stats[m, 0] = n

    times = alternate({"kernel_normalise": lambda: nz.normalise(raw_b[0], row_out), "torch_normalise": torch_normalise,
                       "kernel_update": lambda: nz.update(raw_b), "torch_update": torch_update}, args.inner)
    row = summary(times)
    row["update_bytes_read"] = raw_b.numel() * 4
    row["kernel_update_gb_per_s_of_min"] = raw_b.numel() * 4 / (min(times["kernel_update"]) * 1e-6) / 1e9
    out["calls_members_%d" % members] = row
    print("members = %d: %s" % (members, json.dumps(row)), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
