#!/usr/bin/env python3
"""What the framework side of a PPO iteration costs, and what rng="philox" puts in its place (GPU box only).
For K in 1, 8, 32 learners on 65 536 envs x horizon 64, in ONE process on one set of buffers:
  stages      the three framework stages -- torch.randn((T, N)); population_permutations (K = 1: torch.randperm, as PPO draws);
              normalise_per_member (K = 1: PPO.update's line) -- and the library call that replaces each (LearnerStreams.noise, .order,
              .standardise), alternating
  trainers    a whole update() and a whole iterate() of PopulationPPO (K = 1: PPO as well) with rng="torch" -- the baseline: the code
              path as it was -- and with rng="philox", alternating
Every line is warmed up, then timed for --repeats repeats of a window of --inner calls with the host clock around a device
synchronise; the file keeps every repeat and min - max.  It also holds, for section 16's open question, the update's remainder: a
whole update() minus its optimiser steps timed alone on the same buffers; and the share of the kernel's normals that are exactly the
float64 model's (tests/models/learner_streams_model.py) rounded to float32.
   python tools/update_prologue_cost.py [--out profiles/r28_learner_streams.json] [--members 1,8,32] [--envs 65536] [--horizon 64]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_learner_streams.json"))
ap.add_argument("--members", default="1,8,32")
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--inner", type=int, default=8, help="calls per timed window")
ap.add_argument("--skip-trainers", action="store_true", help="the stages only")
args = ap.parse_args()

import numpy as np
import torch
import pcc_rl_amd
from pcc_rl_amd import build as pbuild
from pcc_rl_amd.ppo import PPO, PopulationPPO, normalise_per_member, population_permutations
from pcc_rl_amd.streams import LearnerStreams

N, T = args.envs, args.horizon
dev = torch.device("cuda:0")
POOLS = (1, 2, 8)   # (as tools/ppo_population.py: the same for every handle, whatever memory is free when it is made)


def timed(fn, inner=None):
    """seconds per call over a window of consecutive calls"""
    inner = inner or args.inner
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def alternate(lines, inner=None):
    """{name: fn} -> {name: {"s": [repeats], "min_max": [min, max]}}: a warm-up of every line, then the lines alternate"""
    times = {name: [] for name in lines}
    for rep in range(-1, args.repeats):
        for name, fn in lines.items():
            t = timed(fn, inner)
            if rep >= 0:
                times[name].append(t)
    return {name: {"s": t, "min_max": [min(t), max(t)]} for name, t in times.items()}


def verdict(row, base, new):
    """Whether `new` beats `base` by more than the baseline's own spread."""
    b, k = row[base]["min_max"], row[new]["min_max"]
    spread = b[1] - b[0]
    return {"baseline": base, "kernel": new, "baseline_spread_s": spread, "gain_s_worst_case": b[0] - k[1],
            "faster_by_more_than_the_baselines_spread": bool(b[0] - k[1] > spread)}


def exact_share():
    """The kernel's normals against the float64 model rounded once: 4 members x 4 096 envs x 16 steps."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "models"))
    import learner_streams_model as model
    K, n_m, Tn = 4, 4096, 16
    st = LearnerStreams(range(K), K * n_m, dev)
    got = st.noise(Tn, 1).cpu().numpy()
    exact = beyond = 0
    for m in range(K):
        want = model.noise64(st.host_keys[m], 1, Tn, n_m)
        want32 = want.astype(np.float32)
        g = got[:, m * n_m:(m + 1) * n_m]
        exact += int((g == want32).sum())
        beyond += int((np.abs(g.astype(np.float64) - want) > np.spacing(np.abs(want32))).sum())
    return {"draws": K * n_m * Tn, "exactly_the_rounded_model": exact, "beyond_one_float32_spacing": beyond, "share_exact": exact / float(K * n_m * Tn)}


out = {"what": "the framework stages of a PPO iteration (noise, minibatch order, advantage standardisation) and the library calls of "
               "rng='philox' that replace them, then whole update() / iterate() calls of both modes, on %d envs x horizon %d; seconds per "
               "call, host clock around a device synchronise, lines alternating, min - max over %d repeats (windows of %d calls) after a "
               "warm-up of each; the baseline is rng='torch' of this build" % (N, T, args.repeats, args.inner),
       "n_envs": N, "horizon": T, "repeats": args.repeats, "calls_per_window": args.inner, "device": torch.cuda.get_device_name(0),
       "build": pbuild.build_info(), "noise_exactness": exact_share(), "members": {}}
print("noise exactness:", json.dumps(out["noise_exactness"]), flush=True)

for K in [int(x) for x in args.members.split(",")]:
    row = {}
    st = LearnerStreams(range(K), N, dev)
    adv = torch.randn((T, N), device=dev) * 3.0 + 1.0
    noise_buf, std_buf = torch.empty((T, N), device=dev), torch.empty((T, N), device=dev)
    perm_buf = torch.empty((K, T * (N // K)), dtype=torch.int64, device=dev)
    flat_adv = adv.reshape(-1)
    lines = {
        "torch_randn": lambda: torch.randn((T, N), device=dev),
        "kernel_noise": lambda: st.noise(T, 1, out=noise_buf),
        "torch_permutations": (lambda: torch.randperm(T * N, device=dev)) if K == 1 else (lambda: population_permutations(T, N, K, device=dev)),
        "kernel_order": lambda: st.order(T, 1, 0, out=perm_buf),
        "torch_standardise": (lambda: (flat_adv - flat_adv.mean()) / (flat_adv.std() + 1e-8)) if K == 1 else (lambda: normalise_per_member(adv, K)),
        "kernel_standardise": lambda: st.standardise(adv, out=std_buf),
    }
    row["stages"] = alternate(lines)
    row["stage_verdicts"] = [verdict(row["stages"], b, k) for b, k in (("torch_randn", "kernel_noise"), ("torch_permutations", "kernel_order"),
                                                                      ("torch_standardise", "kernel_standardise"))]
    del lines, adv, noise_buf, std_buf, perm_buf, flat_adv, st
    torch.cuda.empty_cache()
    print("K = %d stages: %s" % (K, json.dumps({n: r["min_max"] for n, r in row["stages"].items()})), flush=True)

    if not args.skip_trainers:
        envs, agents = {}, {}
        kinds = [("population", PopulationPPO)] + ([("ppo", PPO)] if K == 1 else [])
        for kind, cls in kinds:
            for rng in ("torch", "philox"):
                e = pcc_rl_amd.BatchedNetworkEnv(N, device=dev, seed=0, ring_pools=POOLS)
                envs[(kind, rng)] = e
                agents[(kind, rng)] = cls(e, K, horizon=T, rng=rng) if cls is PopulationPPO else cls(e, horizon=T, rng=rng)
        batches = {k: a.collect() for k, a in agents.items()}
        lines = {}
        for (kind, rng), a in agents.items():
            lines["%s_update_%s" % (kind, rng)] = (lambda a=a, k=(kind, rng): a.update(*batches[k][:5]))
        for (kind, rng), a in agents.items():
            lines["%s_iterate_%s" % (kind, rng)] = a.iterate

        # the update's optimiser steps alone, on the rollout the update() lines use: what is left of update() is its framework side
        pop = agents[("population", "torch")]
        b = batches[("population", "torch")]
        n = T * N
        obs_f, act_f = b[0].reshape(n, -1).contiguous(), b[1].reshape(n).contiguous()
        logp_f, ret_f, adv_f = b[2].reshape(n).contiguous(), b[4].reshape(n).contiguous(), normalise_per_member(b[3], K).reshape(n)
        perm = population_permutations(T, N, K, device=dev)
        per_member = T * (N // K)

        def steps_alone():
            for _ in range(pop.epochs):
                for i in range(0, per_member, pop.minibatch):
                    pop.minibatch_step(obs_f, act_f, logp_f, adv_f, ret_f, perm, i, min(pop.minibatch, per_member - i))
        lines["population_optimiser_steps_alone"] = steps_alone
        row["trainers"] = alternate(lines, inner=max(2, args.inner // 2))
        tr = row["trainers"]
        row["trainer_verdicts"] = [verdict(tr, "%s_%s_torch" % (kind, what), "%s_%s_philox" % (kind, what)) for kind, _ in kinds
                                   for what in ("update", "iterate")]
        u, s = tr["population_update_torch"]["min_max"], tr["population_optimiser_steps_alone"]["min_max"]
        row["update_remainder_torch_s"] = [u[0] - s[1], u[1] - s[0]]
        u = tr["population_update_philox"]["min_max"]
        row["update_remainder_philox_s"] = [u[0] - s[1], u[1] - s[0]]
        row["optimiser_steps_per_update"] = pop.epochs * -(-per_member // pop.minibatch)
        row["framework_stages_per_update_s"] = [row["stages"]["torch_permutations"]["min_max"][i] * pop.epochs +
                                                row["stages"]["torch_standardise"]["min_max"][i] for i in (0, 1)]
        print("K = %d trainers: %s" % (K, json.dumps({n: r["min_max"] for n, r in tr.items()})), flush=True)
        for e in envs.values():
            e.close()
        del envs, agents, batches, lines, pop, b, obs_f, act_f, logp_f, ret_f, adv_f, perm
        torch.cuda.empty_cache()
    out["members"][str(K)] = row

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
