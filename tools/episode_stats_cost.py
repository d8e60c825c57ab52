#!/usr/bin/env python3
"""What the episode ledger costs (GPU box only), in one process --
  (a) calls      pcc_episode_update_pop on one rollout's rows at --envs x --horizon for 1 and --members members: C = 1 (reward and
                 done rows alone) and C = 6 with step records; next to it a device copy of the bytes the call reads (the step
                 records are read as whole 152-byte rows: every cache line of them is touched), and the same accounting in torch
                 (cumulative sums along the steps and masks: per-episode totals by differences of the cumulative sum at the
                 episode ends, per-member sums by a reshape)
  (b) iterate    PPO.iterate() with and without track_episodes
The variants of each group alternate, --repeats repeats after a warm-up of each, a host clock around a device synchronise.
Microseconds per call, min - max over the repeats.
   python tools/episode_stats_cost.py [--out profiles/r20_episode_ledger.json] [--envs 65536] [--horizon 64] [--members 8]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r20_episode_ledger.json"))
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--members", type=int, default=8)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--inner", type=int, default=20, help="calls per timed window of (a)")
ap.add_argument("--iterate-inner", type=int, default=2, help="iterate() calls per timed window of (b)")
args = ap.parse_args()

import torch
import pcc_rl_amd
from pcc_rl_amd import build as pbuild
from pcc_rl_amd.episodes import EpisodeLedger
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
out = {"what": "microseconds per call, host clock around a device synchronise, the variants of a group alternating, %d repeats after a "
               "warm-up of each: (a) the ledger's call on %d envs x %d steps next to a device copy of the bytes it reads and the same "
               "accounting in torch, windows of %d calls; (b) PPO.iterate() with and without track_episodes, windows of %d calls"
               % (args.repeats, N, T, args.inner, args.iterate_inner),
       "device": torch.cuda.get_device_name(0), "build": pbuild.build_info(), "repeats": args.repeats, "n_envs": N, "horizon": T, "members": K}

# (a) ---------------------------------------------------------------------------------------------------------------------
g = torch.Generator(device=dev).manual_seed(1)
rew = torch.randn((T, N), device=dev, generator=g) * 3.0
done = (torch.rand((T, N), device=dev, generator=g) < 0.05).to(torch.uint8)
steps = torch.randn((T, N, 19), device=dev, generator=g, dtype=torch.float64)
CHANNELS = ("sent", "acked", "lost", "run_dur", "latency_ratio")
cols = [0, 1, 2, 5, 17]
small_src = torch.empty(rew.numel() * 4 + done.numel(), dtype=torch.uint8, device=dev)
small_dst = torch.empty_like(small_src)
steps_dst = torch.empty_like(steps)

for members in sorted({1, K}):
    n_m = N // members
    led1 = EpisodeLedger(N, members, device=dev)
    led6 = EpisodeLedger(N, members, CHANNELS, device=dev)

    def torch_ledger(x, carry, totals):
        """x [T][N][C] float64: per-episode totals from the cumulative sum along the steps, per-member sums (no min / max, no last)"""
        C = x.shape[2]
        d = done.bool()
        cum = torch.cumsum(x, dim=0) + carry                                            # the running total, the carry included
        idx = torch.arange(T, device=dev).view(T, 1).expand(T, N)
        last_end = torch.cummax(torch.where(d, idx, torch.full_like(idx, -1)), dim=0)[0]   # the latest end at or before step t; -1: none
        prev_end = torch.cat([torch.full_like(last_end[:1], -1), last_end[:-1]])        # ... before step t
        at = lambda e: torch.where((e >= 0).unsqueeze(-1), torch.gather(cum, 0, e.clamp(min=0).unsqueeze(-1).expand(-1, -1, C)),
                                   torch.zeros((), dtype=cum.dtype, device=dev))
        v = torch.where(d.unsqueeze(-1), cum - at(prev_end), torch.zeros((), dtype=cum.dtype, device=dev))   # an episode's total, at its end
        totals[:, 0] += d.view(T, members, n_m).sum(dim=(0, 2))
        totals[:, 1:1 + C] += v.view(T, members, n_m, C).sum(dim=(0, 2))
        totals[:, 1 + C:] += (v * v).view(T, members, n_m, C).sum(dim=(0, 2))
        carry.copy_(cum[-1] - at(last_end[-1:])[0])

    c1, t1 = torch.zeros((N, 1), dtype=torch.float64, device=dev), torch.zeros((members, 3), dtype=torch.float64, device=dev)
    c6, t6 = torch.zeros((N, 6), dtype=torch.float64, device=dev), torch.zeros((members, 13), dtype=torch.float64, device=dev)

    def torch_c1():
        torch_ledger(rew.double().unsqueeze(-1), c1, t1)

    def torch_c6():
        torch_ledger(torch.cat([rew.double().unsqueeze(-1), steps[:, :, cols]], dim=2), c6, t6)

    times = alternate({"ledger_c1": lambda: led1.update(rew, done), "copy_c1_bytes": lambda: small_dst.copy_(small_src),
                       "torch_c1": torch_c1,
                       "ledger_c6": lambda: led6.update(rew, done, steps), "copy_c6_bytes": lambda: (small_dst.copy_(small_src), steps_dst.copy_(steps)),
                       "torch_c6": torch_c6}, args.inner)
    row = summary(times)
    row["c1_bytes_read"] = small_src.numel()
    row["c6_bytes_read"] = small_src.numel() + steps.numel() * 8
    row["ledger_c1_gb_per_s_of_min"] = row["c1_bytes_read"] / (min(times["ledger_c1"]) * 1e-6) / 1e9
    row["ledger_c6_gb_per_s_of_min"] = row["c6_bytes_read"] / (min(times["ledger_c6"]) * 1e-6) / 1e9
    row["episodes_counted"] = led1.summary()["episodes"]
    # (both ran the same number of calls on the same rows: the torch restatement counts and sums what the ledger does)
    row["torch_counts_the_same_episodes"] = bool(torch.equal(t6[:, 0], led6.totals()[:, 0]))
    row["torch_vs_ledger_sums_max_rel_diff"] = float(((t6[:, 1:7] - led6.totals()[:, 2::4]).abs() / led6.totals()[:, 2::4].abs().clamp(min=1e-300)).max())
    out["calls_members_%d" % members] = row
    print("members = %d: %s" % (members, json.dumps(row)), flush=True)
    del led1, led6, c1, t1, c6, t6
del steps, steps_dst
torch.cuda.empty_cache()

# (b) ---------------------------------------------------------------------------------------------------------------------
envs = [pcc_rl_amd.BatchedNetworkEnv(N, device=dev, seed=0, ring_pools=(1, 2, 8)) for _ in range(2)]
plain, tracked = PPO(envs[0], horizon=T), PPO(envs[1], horizon=T, track_episodes=True)
times = alternate({"iterate_plain": plain.iterate, "iterate_tracked": tracked.iterate}, args.iterate_inner)
for e in envs:
    e.check_flags()
    e.close()
row = summary(times)
row["added_us_of_min"] = min(times["iterate_tracked"]) - min(times["iterate_plain"])
row["plain_spread_us"] = max(times["iterate_plain"]) - min(times["iterate_plain"])
row["tracked_min_inside_plain_spread"] = bool(min(times["iterate_tracked"]) <= max(times["iterate_plain"]))
out["iterate_ppo"] = row
print("iterate: %s" % json.dumps(row), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
