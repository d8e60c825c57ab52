#!/usr/bin/env python3
"""What the step between two generations costs (GPU box only), three things in one process --
  (a) evolve       one pcc_pbt_evolve launch on [K][3 136] blocks (the reference policy: 3 075 parameters), n_cut = K / 4, for K in
                   8, 32, 1024; at K = 8 also PopulationPPO.evolve itself (the launch plus its Python: two small uploads, two allocations)
  (b) framework    what a user did by hand: scores.tolist(), a host sort, index_copy_ on the three blocks, the hyper arithmetic in torch
  (c) iterate      one PopulationPPO.iterate() at --envs x --horizon with K = 8, for scale
(a) and (b) in windows of --inner calls after a warm-up of each, the variants alternating, --repeats repeats, a host clock around a
device synchronise; (c) in windows of --iterate-inner iterations.  Microseconds per call, min - max over the repeats.
   python tools/pbt_cost.py [--out profiles/r14_pbt_cost.json] [--members 8,32,1024] [--envs 65536] [--horizon 64]"""
import argparse, json, os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r14_pbt_cost.json"))
ap.add_argument("--members", default="8,32,1024")
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--inner", type=int, default=100, help="calls per timed window of (a) and (b)")
ap.add_argument("--iterate-inner", type=int, default=4, help="iterate() calls per timed window of (c) (an iteration is tens of milliseconds)")
args = ap.parse_args()

import torch
import pcc_rl_amd
from pcc_rl_amd import build as pbuild
from pcc_rl_amd.env import _ptr
from pcc_rl_amd.native import lib
from pcc_rl_amd.ppo import PopulationPPO, explore_matrix

dev = torch.device("cuda:0")
N_PARAMS, STRIDE = 3075, 3136
EX_ROWS = explore_matrix()
stream = lambda: torch.cuda.current_stream(dev).cuda_stream


class Blocks(object):
    def __init__(self, K):
        g = torch.Generator(device=dev).manual_seed(K)
        self.K, self.cut = K, K // 4
        self.P, self.M, self.V = (torch.randn((K, STRIDE), device=dev, generator=g) for _ in range(3))
        self.H = torch.rand((K, 8), device=dev, generator=g) + 0.5
        self.score = torch.randn(K, device=dev, generator=g, dtype=torch.float64)
        self.ex = torch.tensor(EX_ROWS, dtype=torch.float32, device=dev)
        self.parent, self.rank = (torch.empty(K, dtype=torch.int32, device=dev) for _ in range(2))
        self.generation, self.rng = 0, random.Random(K)

    def evolve(self):   # (a)
        rc = lib().pcc_pbt_evolve(_ptr(self.score), self.K, self.cut, _ptr(self.P), _ptr(self.M), _ptr(self.V), STRIDE, N_PARAMS, _ptr(self.H),
                                  _ptr(self.ex), 0, self.generation, _ptr(self.parent), _ptr(self.rank), stream())
        assert rc == 0, rc
        self.generation += 1

    def framework(self):   # (b)
        s = self.score.tolist()
        order = sorted(range(self.K), key=lambda i: (-s[i], i))
        dst = order[self.K - self.cut:]
        src = [order[self.rng.randrange(self.cut)] for _ in dst]
        si, di = torch.tensor(src, device=dev), torch.tensor(dst, device=dev)
        for B in (self.P, self.M, self.V):
            B.index_copy_(0, di, B.index_select(0, si))
        f = torch.tensor([[EX_ROWS[c][self.rng.getrandbits(1)] for c in range(8)] for _ in dst], dtype=torch.float32, device=dev)
        self.H.index_copy_(0, di, torch.minimum(torch.maximum(self.H.index_select(0, si) * f, self.ex[:, 2]), self.ex[:, 3]))


def timed(fn, inner):
    """microseconds per call over a window of `inner` consecutive calls"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e6


out = {"what": "microseconds per call, host clock around a device synchronise, windows of %d calls (iterate: %d) after a warm-up of each variant, "
               "the variants alternating, %d repeats: (a) one pcc_pbt_evolve launch on [K][%d] blocks (%d parameters), n_cut = K / 4; (b) the same step "
               "by hand: scores.tolist(), a host sort, index_copy_ on the three blocks, the hyper arithmetic in torch; (c) one PopulationPPO.iterate() "
               "of %d envs x %d steps, K = 8, and PopulationPPO.evolve on that population" % (args.inner, args.iterate_inner, args.repeats, STRIDE, N_PARAMS, args.envs, args.horizon),
       "device": torch.cuda.get_device_name(0), "build": pbuild.build_info(), "repeats": args.repeats, "calls_per_window": args.inner, "members": {}}
for K in [int(x) for x in args.members.split(",")]:
    b = Blocks(K)
    times = {"evolve": [], "framework": []}
    for rep in range(-1, args.repeats):   # -1: the warm-up of both
        for name in times:
            t = timed(getattr(b, name), args.inner)
            if rep >= 0:
                times[name].append(t)
    out["members"][str(K)] = {"n_cut": b.cut, "evolve_us": times["evolve"], "framework_us": times["framework"],
                              "evolve_us_min_max": [min(times["evolve"]), max(times["evolve"])],
                              "framework_us_min_max": [min(times["framework"]), max(times["framework"])]}
    print("K = %d: %s" % (K, json.dumps(out["members"][str(K)])), flush=True)

env = pcc_rl_amd.BatchedNetworkEnv(args.envs, device=dev, seed=0, ring_pools=(1, 2, 8))
pop = PopulationPPO(env, 8, horizon=args.horizon)
scores = [0.0] * 8


def iterate():
    scores[:] = pop.iterate()["mean_step_reward"]


it_us, ev_us = [], []
for rep in range(-1, args.repeats):
    a, e = timed(iterate, args.iterate_inner), timed(lambda: pop.evolve(scores), args.inner)
    if rep >= 0:
        it_us.append(a)
        ev_us.append(e)
env.check_flags()
out["population_k8"] = {"iterate_us": it_us, "iterate_us_min_max": [min(it_us), max(it_us)], "method_evolve_us": ev_us,
                        "method_evolve_us_min_max": [min(ev_us), max(ev_us)], "n_envs": args.envs, "horizon": args.horizon}
print("K = 8 population: %s" % json.dumps(out["population_k8"]), flush=True)
env.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("wrote", args.out)
