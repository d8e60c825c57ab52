#!/usr/bin/env python3
"""What time-limit bootstrapping costs (GPU box only), four things, the first three in one process --
  (a) terminal     pcc_terminal_obs alone on one rollout's rows at every --envs size: in lockstep (one burst: every env done on the
                   same row) and staggered (every env's 400-step episode at its own phase: about horizon / 400 of the envs have a done,
                   spread over the rows).  What it must read: the horizon x envs done bytes, and per done H F floats and F doubles; what
                   it must write: slots x envs x H F floats and a count per env.  Next to it the time to read the done bytes once at
                   the device's streaming rate, the rate taken from a 1 GiB copy in the same windows
  (b) gae          pcc_gae_boot against pcc_gae on the same rows (the staggered dones; pcc_gae ignores the terminal values)
  (c) collect      PPO.collect() with bootstrap_time_limit off -- the calls of before the option, nothing else -- and on: the step
                   records every env step now stores are in this difference (--no-collect leaves it out)
  (d) curves       with --curves: examples/learning_curve.py twice as child processes, same seed, without and with
                   --bootstrap-time-limit; the value loss of the last iterations and the held-out return of each
The variants of each group alternate, --repeats repeats after a warm-up of each, a host clock around a device synchronise.
Microseconds per call, min - max over the repeats.
   python tools/time_limit_cost.py [--out profiles/r29_time_limit.json] [--envs 65536,262144] [--horizon 64] [--curves]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_time_limit.json"))
ap.add_argument("--envs", default="65536,262144")
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--inner", type=int, default=50, help="calls per timed window of (a) and (b)")
ap.add_argument("--collect-inner", type=int, default=2, help="collect() calls per timed window of (c)")
ap.add_argument("--no-collect", action="store_true")
ap.add_argument("--curves", action="store_true")
ap.add_argument("--curve-env-steps", type=float, default=2e8)
ap.add_argument("--curve-timeout", type=int, default=900, help="seconds for each child process of (d)")
args = ap.parse_args()

import torch
import pcc_rl_amd
from pcc_rl_amd import build as pbuild
from pcc_rl_amd import timelimit
from pcc_rl_amd.ppo import PPO, gae_fused

dev = torch.device("cuda:0")
MAX_STEPS = 400


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
out = {"what": "microseconds per call, host clock around a device synchronise, the variants of a group alternating, %d repeats after a "
               "warm-up of each: (a) pcc_terminal_obs on [%d][envs] rows, windows of %d calls; (b) pcc_gae_boot and pcc_gae on the same "
               "rows, windows of %d calls; (c) PPO.collect() without and with bootstrap_time_limit, windows of %d calls; (d) two learning "
               "curves" % (args.repeats, T, args.inner, args.inner, args.collect_inner),
       "device": torch.cuda.get_device_name(0), "build": pbuild.build_info(), "repeats": args.repeats, "horizon": T}

# (a), (b) ----------------------------------------------------------------------------------------------------------------
g = torch.Generator(device=dev).manual_seed(1)
big = torch.empty(1 << 28, device=dev)          # 1 GiB: its copy reads and writes 1 GiB each
big_to = torch.empty_like(big)
for N in [int(x) for x in args.envs.split(",")]:
    env = pcc_rl_amd.BatchedNetworkEnv(N, device=dev, seed=0, ring_pools=(1, 2, 8))   # (for its features; never stepped)
    D, F = env.obs_dim, len(env.feature_ids)
    obs_b = torch.rand((T + 1, N, D), device=dev, generator=g)
    steps_b = torch.rand((T, N, 19), device=dev, generator=g, dtype=torch.float64)
    rew_b = torch.randn((T, N), device=dev, generator=g)
    val_b = torch.randn((T, N), device=dev, generator=g)
    last_v = torch.randn(N, device=dev, generator=g)
    rows = torch.arange(T, device=dev)[:, None]
    phase = torch.randint(0, MAX_STEPS, (N,), device=dev, generator=g)
    dones = {"lockstep": (rows == T // 2).expand(T, N).contiguous(),
             "staggered": ((rows + phase[None, :]) % MAX_STEPS == MAX_STEPS - 1).contiguous()}
    n_slots = timelimit.slots(T, MAX_STEPS)
    outs = (torch.empty((n_slots, N, D), device=dev), torch.empty(N, dtype=torch.int32, device=dev))
    term_val = torch.randn((n_slots, N), device=dev, generator=g)
    tl = timelimit.TimeLimitBootstrap(env, T)
    tl.term_val.copy_(term_val)
    variants = {"copy_1gib": (lambda: big_to.copy_(big), 5)}
    for kind, d in dones.items():
        variants["terminal_" + kind] = (lambda d=d: timelimit.terminal_observations(env, obs_b, steps_b, d, n_slots, out=outs), args.inner)
    timelimit.terminal_observations(env, obs_b, steps_b, dones["staggered"], n_slots, out=(tl.term_obs, tl.term_count))
    variants["gae"] = (lambda: gae_fused(rew_b, val_b, dones["staggered"], last_v, 0.99, 0.95), args.inner)
    variants["gae_boot"] = (lambda: tl.gae(rew_b, val_b, dones["staggered"], last_v, 0.99, 0.95), args.inner)
    times = alternate(variants)
    row = summary(times)
    stream = 2.0 * big.numel() * 4 / (min(times["copy_1gib"]) * 1e-6)            # bytes per second, read + write
    row["streaming_gb_per_s_of_min"] = stream / 1e9
    row["done_bytes"] = T * N
    row["done_rows_once_at_streaming_rate_us"] = T * N / stream * 1e6
    for kind, d in dones.items():
        hits = int(d.sum())
        row[kind + "_dones"] = hits
        row[kind + "_bytes_read"] = T * N + hits * (D * 4 + F * 8)
        row[kind + "_bytes_written"] = n_slots * N * D * 4 + N * 4
        t_min = min(times["terminal_" + kind]) * 1e-6
        row["terminal_%s_gb_per_s_read_of_min" % kind] = row[kind + "_bytes_read"] / t_min / 1e9
        row["terminal_%s_gb_per_s_read_and_written_of_min" % kind] = (row[kind + "_bytes_read"] + row[kind + "_bytes_written"]) / t_min / 1e9
    row["gae_boot_minus_gae_us_of_min"] = min(times["gae_boot"]) - min(times["gae"])
    row["gae_spread_us"] = max(times["gae"]) - min(times["gae"])
    out["calls_envs_%d" % N] = row
    print("envs = %d: %s" % (N, json.dumps(row)), flush=True)
    env.close()
    del env, tl, obs_b, steps_b, rew_b, val_b, outs, dones
    torch.cuda.empty_cache()
del big, big_to
torch.cuda.empty_cache()

# (c) ---------------------------------------------------------------------------------------------------------------------
# lr = 0 is not needed here: collect() alone never updates, so the two trainers run the same policy on envs of the same seed.
if not args.no_collect:
    for N in [int(x) for x in args.envs.split(",")]:
        envs = [pcc_rl_amd.BatchedNetworkEnv(N, device=dev, seed=0, ring_pools=(1, 2, 8)) for _ in range(2)]
        off, on = (PPO(e, horizon=T, seed=0, bootstrap_time_limit=b) for e, b in zip(envs, (False, True)))
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

# (d) ---------------------------------------------------------------------------------------------------------------------
if args.curves:
    torch.cuda.synchronize()
    curves = {}
    for name, flags in (("plain", []), ("bootstrap_time_limit", ["--bootstrap-time-limit"])):
        cmd = [sys.executable, os.path.join(ROOT, "examples", "learning_curve.py"), "--seed", "0", "--env-steps", str(args.curve_env_steps)] + flags
        res = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, timeout=args.curve_timeout)
        if res.returncode != 0:
            raise SystemExit("%s failed (%d)" % (" ".join(cmd), res.returncode))
        r = json.loads(res.stdout[res.stdout.index("{"):])
        tail = r["curve"][-max(1, len(r["curve"]) // 10):]
        curves[name] = {"training": r["training"], "value_loss_first": r["curve"][0]["value_loss"],
                        "value_loss_mean_of_last_tenth": sum(c["value_loss"] for c in tail) / len(tail),
                        "held_out": {h["controller"]: h["mean_episode_return"] for h in r["held_out_evaluation"]}}
        print("%s: %s" % (name, json.dumps(curves[name])), flush=True)
    out["learning_curves"] = curves

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
