#!/usr/bin/env python3
"""What one launch for K members buys (GPU box only): K PPO learners on 65 536 envs, horizon 64, three ways --
  (a) population      PopulationPPO as built: one env handle, one library call for all members per forward / GAE / optimiser step
  (b) member_calls    the same class with its three library calls replaced by the single-policy entry points, member by member (MemberCalls below)
  (c) k_handles       what a user did before: K PPO objects on K handles of 65 536 / K envs, iterated one after another
for K in 1, 8, 32 (K = 1 is the control: the three must agree within their own spread).  One process; every variant is warmed
up, then the variants alternate for three repeats; a repeat times a window of --inner rollouts and a window of --inner updates
(of the last rollout) with a host clock around a device synchronise; seconds per iteration, min - max over the repeats.
   python tools/ppo_population.py [--out profiles/r13_ppo_population.json] [--members 1,8,32] [--envs 65536] [--horizon 64] [--repeats 3]
   rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ppo_population.py --trace-run 8     # kernel times: (a) alone, two iterations
   python tools/ppo_population.py --merge-kernel-stats DIR/.../*_kernel_stats.csv --out FILE       # fold those into FILE"""
import argparse, csv, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r13_ppo_population.json"))
ap.add_argument("--members", default="1,8,32")
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--inner", type=int, default=8, help="collect() calls, then update() calls, per timed window (an iteration is tens of milliseconds)")
ap.add_argument("--trace-run", type=int, default=0, help="K: run variant (a) alone for two iterations and write nothing (for rocprofv3)")
ap.add_argument("--merge-kernel-stats", default="", help="a rocprofv3 kernel_stats.csv of a --trace-run: its PPO-stage kernels go into --out")
args = ap.parse_args()

if args.merge_kernel_stats:
    with open(args.out) as f:
        out = json.load(f)
    rows = []
    with open(args.merge_kernel_stats) as f:
        for r in csv.DictReader(f):
            name = r.get("Name", "")
            if any(k in name for k in ("policy_act_", "ppo_grad_", "ppo_adam_kernel", "gae_kernel")):   # the PPO-stage kernels (both entry points')
                rows.append({"kernel": name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0], "calls": int(r["Calls"]),
                             "total_us": float(r["TotalDurationNs"]) / 1e3, "mean_us": float(r["AverageNs"]) / 1e3,
                             "share_of_gpu_time_pct": float(r["Percentage"])})
    out["kernel_trace"] = {"what": "rocprofv3 --kernel-trace --stats, a run of its own: variant (a), two iterations", "kernels": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    sys.exit(0)

import torch
import pcc_rl_amd
from pcc_rl_amd import build as pbuild
from pcc_rl_amd.env import _ptr
from pcc_rl_amd.native import lib
from pcc_rl_amd.ppo import PPO, PopulationPPO, gae_fused

N, T = args.envs, args.horizon
dev = torch.device("cuda:0")
POOLS = (1, 2, 8)   # the same for every handle, whatever memory is free when it is made: ~32 GB per 65 536 envs, three sets alive at
                    # once (the least pools, 2, 8, 32, ran dry under the untrained policies' N(0, 1) actions at this size)


def make_env(n, base=0):
    return pcc_rl_amd.BatchedNetworkEnv(n, device=dev, seed=0, env_gid_base=base, ring_pools=POOLS)


class MemberCalls(PopulationPPO):
    """Variant (b): PopulationPPO's three library calls replaced by the single-policy entry points, member by member -- the
    same env handle, buffers, permutations and (bit for bit) results; only the number of launches differs."""

    def _act(self, obs, noise, act, logp, val):
        n, D = self.n_member, obs.shape[1]
        sl = lambda x, m: None if x is None else x[m * n:(m + 1) * n]
        for m in range(self.members):
            rc = lib().pcc_policy_act(_ptr(sl(obs, m)), n, D, _ptr(self.flat[m]), self.arch[0], self.arch[1], _ptr(sl(noise, m)), None,
                                      _ptr(sl(act, m)), _ptr(sl(logp, m)), _ptr(sl(val, m)), self._stream())
            assert rc == 0, rc

    def _gae(self, rew_b, val_b, done_b, last_v):   # (pcc_gae takes contiguous rows: a member's columns are copied out and back)
        adv, ret = torch.empty_like(rew_b), torch.empty_like(rew_b)
        n = self.n_member
        for m in range(self.members):
            c = slice(m * n, (m + 1) * n)
            adv[:, c], ret[:, c] = gae_fused(rew_b[:, c], val_b[:, c], done_b[:, c], last_v[c], self.hyper_rows[m][3], self.hyper_rows[m][4])
        return adv, ret

    def minibatch_step(self, obs_f, act_f, logp_f, adv_f, ret_f, perm, start, count, grad_out=None):
        self.adam_t += 1
        for m in range(self.members):
            h = self.hyper_rows[m]
            rc = lib().pcc_ppo_minibatch_step(_ptr(obs_f), _ptr(act_f), _ptr(logp_f), _ptr(adv_f), _ptr(ret_f), _ptr(perm[m]), start, count,
                                              obs_f.shape[1], self.arch[0], self.arch[1], _ptr(self.flat[m]), _ptr(self.adam_m[m]),
                                              _ptr(self.adam_v[m]), self.adam_t, h[0], 0.9, 0.999, self.adam_eps, h[1], h[2],
                                              _ptr(self.scratch[m * self.scratch_floats:]), None, _ptr(self.stats_buf[m]), self._stream())
            assert rc == 0, rc


class Population(object):   # (a), and (b) with member_calls
    def __init__(self, K, member_calls):
        self.env = make_env(N)
        self.pop = (MemberCalls if member_calls else PopulationPPO)(self.env, K, horizon=T)

    def collect(self):
        self.batch = self.pop.collect()

    def update(self):
        self.pop.update(*self.batch[:5])

    def close(self):
        self.env.close()


class Handles(object):      # (c)
    def __init__(self, K):
        self.envs = [make_env(N // K, m * (N // K)) for m in range(K)]
        self.agents = [PPO(e, horizon=T, seed=m) for m, e in enumerate(self.envs)]

    def collect(self):
        self.batches = [a.collect() for a in self.agents]

    def update(self):
        for a, b in zip(self.agents, self.batches):
            a.update(*b[:5])

    def close(self):
        for e in self.envs:
            e.close()


def timed(fn):
    """seconds per call over a window of --inner consecutive calls"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.inner


if args.trace_run:
    v = Population(args.trace_run, False)
    for _ in range(2):
        v.collect()
        v.update()
    torch.cuda.synchronize()
    v.close()
    sys.exit(0)

out = {"what": "K PPO learners on %d envs x horizon %d: (a) PopulationPPO, (b) the same through the single-policy entry points member by "
               "member, (c) K PPO objects on K handles of N / K envs; seconds per iteration, host clock around a device synchronise, "
               "variants alternating, min - max over %d repeats (windows of %d calls) after a warm-up of each" % (N, T, args.repeats, args.inner),
       "n_envs": N, "horizon": T, "repeats": args.repeats, "calls_per_window": args.inner, "device": torch.cuda.get_device_name(0), "build": pbuild.build_info(), "members": {}}
for K in [int(x) for x in args.members.split(",")]:
    variants = {"population": Population(K, False), "member_calls": Population(K, True), "k_handles": Handles(K)}
    times = {name: {"t_roll": [], "update_s": []} for name in variants}
    for rep in range(-1, args.repeats):   # -1: the warm-up of every variant
        for name, v in variants.items():
            tr, tu = timed(v.collect), timed(v.update)
            if rep >= 0:
                times[name]["t_roll"].append(tr)
                times[name]["update_s"].append(tu)
    row = {}
    for name, t in times.items():
        total = [a + b for a, b in zip(t["t_roll"], t["update_s"])]
        row[name] = {"t_roll_s": t["t_roll"], "update_s": t["update_s"], "t_roll_min_max": [min(t["t_roll"]), max(t["t_roll"])],
                     "update_min_max": [min(t["update_s"]), max(t["update_s"])],
                     "env_steps_per_s_incl_learning_min_max": [N * T / max(total), N * T / min(total)]}
    row["minibatch_per_member"] = variants["population"].pop.minibatch
    row["optimiser_steps_per_iteration"] = variants["population"].pop.epochs * -(-T * (N // K) // variants["population"].pop.minibatch)
    out["members"][str(K)] = row
    print("K = %d: %s" % (K, json.dumps({n: (r["t_roll_min_max"], r["update_min_max"]) for n, r in row.items() if isinstance(r, dict)})), flush=True)
    for v in variants.values():
        v.close()
    del variants
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
