#!/usr/bin/env python3
"""What a reward objective costs (GPU box only), three things in one process --
  (a) call       pcc_reward_objective_pop alone on one rollout's step records at every --envs size: the reference weights (three
                 columns read), all six weights, and the reference weights over 8 members.  What it must read: every 128-byte line of
                 the records (a lane's row is 152 bytes from its neighbour's: whichever columns are read, every line is fetched), T N
                 152 bytes; what it writes: T N 4 bytes.  Next to it the device's streaming rate from a 1 GiB copy in the same windows
  (b) torch      the same arithmetic with framework launches: column indexing, float64 products and sums, the scale, the cast
  (c) collect    PPO.collect() with objective=None -- the calls of before the option, nothing else -- and with the reference
                 objective: the step records every env step now stores and the call are in this difference (--no-collect leaves it
                 out)
The variants of each group alternate, --repeats repeats after a warm-up of each, a host clock around a device synchronise.
Microseconds per call, min - max over the repeats.
   python tools/reward_objective_cost.py [--out profiles/r30_reward_objective.json] [--envs 65536,262144] [--horizon 64]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_reward_objective.json"))
ap.add_argument("--envs", default="65536,262144")
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--inner", type=int, default=20, help="calls per timed window of (a) and (b)")
ap.add_argument("--collect-inner", type=int, default=2, help="collect() calls per timed window of (c)")
ap.add_argument("--no-collect", action="store_true")
args = ap.parse_args()

import torch
import pcc_rl_amd
from pcc_rl_amd import build as pbuild
from pcc_rl_amd.objective import RewardObjective
from pcc_rl_amd.ppo import PPO

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


def torch_reward(steps_b, w):
    """The reference objective's arithmetic as framework launches: float64 columns, the env's operations, one cast."""
    acc = (w[0] * steps_b[..., 8]) / 12000.0 + w[1] * steps_b[..., 11] + w[2] * steps_b[..., 12]
    return (acc * 0.001).float()


T = args.horizon
ALL_SIX = (3.0, -700.0, -1500.0, -40.0, -0.25, 1.5)
out = {"what": "microseconds per call, host clock around a device synchronise, the variants of a group alternating, %d repeats after a "
               "warm-up of each: (a) pcc_reward_objective_pop on [%d][envs][19] float64 records, windows of %d calls; (b) the same "
               "arithmetic as torch launches; (c) PPO.collect() with objective=None and with the reference objective, windows of %d "
               "calls" % (args.repeats, T, args.inner, args.collect_inner),
       "device": torch.cuda.get_device_name(0), "build": pbuild.build_info(), "repeats": args.repeats, "horizon": T}

# (a), (b) ----------------------------------------------------------------------------------------------------------------
g = torch.Generator(device=dev).manual_seed(1)
big = torch.empty(1 << 28, device=dev)          # 1 GiB: its copy reads and writes 1 GiB each
big_to = torch.empty_like(big)
for N in [int(x) for x in args.envs.split(",")]:
    steps_b = torch.rand((T, N, 19), device=dev, generator=g, dtype=torch.float64)
    rew = torch.empty((T, N), device=dev)
    objs = {"call_reference": RewardObjective(N, 1, None, device=dev), "call_all_six": RewardObjective(N, 1, ALL_SIX, device=dev),
            "call_reference_8_members": RewardObjective(N, 8, None, device=dev)}
    w = [10.0, -1e3, -2e3]
    same = bool(torch.equal(objs["call_reference"].apply(steps_b), torch_reward(steps_b, w)))   # (the framework may divide by multiplying)
    variants = {"copy_1gib": (lambda: big_to.copy_(big), 5)}
    for name, o in objs.items():
        variants[name] = (lambda o=o: o.apply(steps_b, out=rew), args.inner)
    variants["torch_reference"] = (lambda: torch_reward(steps_b, w), args.inner)
    times = alternate(variants)
    row = summary(times)
    row["torch_bits_equal_the_call"] = same
    stream = 2.0 * big.numel() * 4 / (min(times["copy_1gib"]) * 1e-6)            # bytes per second, read + write
    row["streaming_gb_per_s_of_min"] = stream / 1e9
    row["bytes_read"], row["bytes_written"] = T * N * 152, T * N * 4
    moved = row["bytes_read"] + row["bytes_written"]
    for name in objs:
        row[name + "_gb_per_s_of_min"] = moved / (min(times[name]) * 1e-6) / 1e9
    row["records_once_at_streaming_rate_us"] = moved / stream * 1e6
    row["torch_over_call_of_min"] = min(times["torch_reference"]) / min(times["call_reference"])
    out["calls_envs_%d" % N] = row
    print("envs = %d: %s" % (N, json.dumps(row)), flush=True)
    del steps_b, rew, objs
    torch.cuda.empty_cache()
del big, big_to
torch.cuda.empty_cache()

# (c) ---------------------------------------------------------------------------------------------------------------------
# collect() alone never updates, so the two trainers run the same policy on envs of the same seed.
if not args.no_collect:
    for N in [int(x) for x in args.envs.split(",")]:
        envs = [pcc_rl_amd.BatchedNetworkEnv(N, device=dev, seed=0, ring_pools=(1, 2, 8)) for _ in range(2)]
        off, on = (PPO(e, horizon=T, seed=0, objective=o) for e, o in zip(envs, (None, RewardObjective.DEFAULT)))
        times = alternate({"collect_off": (off.collect, args.collect_inner), "collect_on": (on.collect, args.collect_inner)})
        for e in envs:
            e.check_flags()
            e.close()
        row = summary(times)
        row["added_us_of_min"] = min(times["collect_on"]) - min(times["collect_off"])
        row["added_fraction_of_min"] = row["added_us_of_min"] / min(times["collect_off"])
        row["step_record_bytes"] = T * N * 19 * 8
        out["collect_envs_%d" % N] = row
        print("collect, envs = %d: %s" % (N, json.dumps(row)), flush=True)
        del off, on, envs
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
