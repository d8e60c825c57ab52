#!/usr/bin/env python3
"""PPO.collect() with the policy kernel + step loop (policy_in_step=False) against the closed-loop call (policy_in_step=True,
pcc_rollout), the two alternating on one handle (GPU box only; medians and minima over the repeats): 65 536 x 64, 262 144 x 64 and config 2 (4 096 envs on the
fixed link) x 400 at the library's own small-batch threshold.  Writes profiles/<name>.json with the commit stamped.

    python tools/rollout_throughput.py [--repeats 3] [--out profiles/rollout_throughput.json]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import pcc_rl_amd
from pcc_rl_amd.ppo import PPO


def commit():
    from pcc_rl_amd import build as pbuild
    return pbuild._source_stamp()   # (the commit of the tree and a hash of the sources: the GPU box has no .git)


def measure(N, T, repeats, **env_kw):
    env = pcc_rl_amd.BatchedNetworkEnv(N, device="cuda", seed=0, **env_kw)
    agents = {False: PPO(env, horizon=T, seed=0), True: PPO(env, horizon=T, seed=0, policy_in_step=True)}
    times = {False: [], True: []}
    for in_step in (False, True):   # warm-up: first launches, the in-step path's action buffers
        agents[in_step].collect()
    for _ in range(repeats):
        for in_step in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agents[in_step].collect()
            torch.cuda.synchronize()
            times[in_step].append(time.perf_counter() - t0)
    env.close()
    row = {"n_envs": N, "horizon": T, "env": env_kw and {k: list(v) if isinstance(v, tuple) else v for k, v in env_kw.items()} or {}}
    for in_step, key in ((False, "policy_kernel_loop"), (True, "policy_in_step")):
        ts = sorted(times[in_step])
        row[key] = {"s_per_collect": ts, "env_steps_per_s_median": N * T / ts[len(ts) // 2],
                    "ms_per_step_median": 1e3 * ts[len(ts) // 2] / T, "ms_per_step_min": 1e3 * ts[0] / T}
    for stat in ("median", "min"):
        row["speedup_" + stat] = row["policy_kernel_loop"]["ms_per_step_" + stat] / row["policy_in_step"]["ms_per_step_" + stat]
    print(json.dumps({k: row[k] for k in ("n_envs", "horizon", "speedup_median", "speedup_min")}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)   # (a collect of 64 steps sees one phase of the 400-step episode: the
                                                        # step cost follows the phase, so a few repeats of each are noise)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_throughput.json"))
    args = ap.parse_args()
    rows = [measure(65536, 64, args.repeats), measure(262144, 64, args.repeats),
            measure(4096, 400, args.repeats, link_params=(200.0, 0.03, 5.0, 0.0, 60.0))]
    out = {"commit": commit(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "what": "PPO.collect(): policy kernel + pcc_step per step (policy_in_step=False) vs one pcc_rollout per horizon "
                   "(policy_in_step=True), alternating on one handle; includes torch.randn of the noise, flat_params and the GAE",
           "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
