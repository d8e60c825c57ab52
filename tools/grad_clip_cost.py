#!/usr/bin/env python3
"""What gradient-norm clipping costs (GPU box only).  A driver and its steps: the driver starts every step as a
fresh process under a time limit of its own, one after the other, stops at the first step that fails and merges what the steps
printed into --out.  The steps --
  update   PPO.update() (kind ppo) or PopulationPPO.update() with --members members (kind population) on ONE collected rollout of
           --envs x --horizon: two objects of the same kind in one process, max_grad_norm=None and max_grad_norm=--limit, the same
           seeds; windows of --inner update() calls, a warm-up window of each, then --repeats windows, the two alternating.  The
           unclipped update's kernels are the parent commit's (the old units' device code is unchanged), so the difference is the
           option's own work: per optimiser step one more library call with three small launches (the hyper copy, the Adam launch
           that returns at lr == 0, the norm + Adam launch) in place of the Adam launch, and one more read-back per update().
  bench    bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline in --tree (the driver: --bench-repeats runs per tree, this tree and
           --parent alternating).  bench.py runs none of the new code.
Milliseconds per update(), host clock around a device synchronise.
   python tools/grad_clip_cost.py [--out profiles/r25_grad_clip.json] [--parent DIR] [--skip bench]"""
import argparse, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_grad_clip.json"))
ap.add_argument("--step", default="", choices=("", "update", "bench"))
ap.add_argument("--kind", default="ppo", choices=("ppo", "population"))
ap.add_argument("--tree", default=ROOT, help="the source tree a step imports the package from (with its own built library)")
ap.add_argument("--parent", default="", help="a checkout of the parent commit with its own built library: bench runs there too")
ap.add_argument("--skip", default="", help="steps the driver leaves out, comma-separated")
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--members", type=int, default=8)
ap.add_argument("--limit", type=float, default=0.5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--inner", type=int, default=3, help="update() calls per timed window")
ap.add_argument("--bench-repeats", type=int, default=3, help="bench.py runs per tree")
ap.add_argument("--step-timeout", type=int, default=240, help="seconds a step may take")
args = ap.parse_args()
MARK = "RESULT_JSON "


def driver():
    skip = set(x for x in args.skip.split(",") if x)
    out = {"what": "tools/grad_clip_cost.py: every step a fresh process under `timeout`, chained; see the tool's docstring",
           "envs": args.envs, "horizon": args.horizon, "repeats": args.repeats, "inner": args.inner, "limit": args.limit}
    common = ["--envs", str(args.envs), "--horizon", str(args.horizon), "--members", str(args.members), "--limit", str(args.limit),
              "--repeats", str(args.repeats), "--inner", str(args.inner)]

    def run(step, tree, extra=()):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--tree", tree] + common + list(extra)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, cwd=tree)
        sys.stdout.write(p.stdout[-3000:])
        if p.returncode != 0:   # a fault, an abort or the time limit: nothing more is started on the GPU
            print("step %s in %s ended with status %d: stopping here" % (step, tree, p.returncode), flush=True)
            save(out)
            sys.exit(1)
        return json.loads([l for l in p.stdout.splitlines() if l.startswith(MARK)][-1][len(MARK):])

    if "update" not in skip:
        out["update_ppo"] = run("update", ROOT, ["--kind", "ppo"])
        out["update_population_k%d" % args.members] = run("update", ROOT, ["--kind", "population"])
    if "bench" not in skip:
        trees = [("this_tree", ROOT)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
        runs = {name: [] for name, _ in trees}
        for _ in range(args.bench_repeats):
            for name, tree in trees:
                runs[name].append(run("bench", tree))
        out["bench"] = {name: {"value": [r["value"] for r in rs], "unit": rs[0].get("unit")} for name, rs in runs.items()}
        if "parent" in runs:
            mine, theirs = sorted(out["bench"]["this_tree"]["value"]), out["bench"]["parent"]["value"]
            out["bench"]["median_inside_parent_min_max"] = bool(min(theirs) <= mine[len(mine) // 2] <= max(theirs))
    save(out)


def save(out):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


def step_update():
    import torch
    import pcc_rl_amd
    from pcc_rl_amd import build as pbuild
    from pcc_rl_amd.ppo import PPO, PopulationPPO
    N, T, K = args.envs, args.horizon, args.members
    made = {}
    for name, limit in (("off", None), ("on", args.limit)):
        env = pcc_rl_amd.BatchedNetworkEnv(N, device="cuda:0", seed=0, ring_pools=(1, 2, 8))
        if args.kind == "ppo":
            agent = PPO(env, horizon=T, seed=0, minibatch=max(2048, N * T // 4), max_grad_norm=limit)
        else:
            agent = PopulationPPO(env, K, horizon=T, max_grad_norm=limit)
        rollout = agent.collect()[:5]
        env.check_flags()
        made[name] = (env, agent, rollout)
    per_update = made["off"][1].epochs * ((N * T // (1 if args.kind == "ppo" else K) + made["off"][1].minibatch - 1) // made["off"][1].minibatch)

    def window(name):
        _, agent, rollout = made[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            stats = agent.update(*rollout)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.inner * 1e3, stats

    times, last = {"off": [], "on": []}, {}
    for rep in range(-1, args.repeats):   # (a warm-up window of each, then the repeats, the two alternating)
        for name in ("off", "on"):
            t, last[name] = window(name)
            if rep >= 0:
                times[name].append(t)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"device": torch.cuda.get_device_name(0), "build": pbuild.build_info(), "unit": "milliseconds per update()", "kind": args.kind,
           "members": 1 if args.kind == "ppo" else K, "optimiser_steps_per_update": per_update,
           "off_ms": times["off"], "on_ms": times["on"], "off_ms_min_max": [min(times["off"]), max(times["off"])],
           "on_ms_min_max": [min(times["on"]), max(times["on"])],
           "added_ms_of_medians": med(times["on"]) - med(times["off"]),
           "added_us_per_optimiser_step_of_medians": (med(times["on"]) - med(times["off"])) * 1e3 / per_update,
           "added_share_of_medians": med(times["on"]) / med(times["off"]) - 1.0,
           "last_update_on": {k: last["on"][k] for k in ("grad_norm", "max_grad_norm_seen", "clipped_steps", "skipped_steps")}}
    print("%s: %s" % (args.kind, json.dumps(out)), flush=True)
    for env, _, _ in made.values():
        env.close()
    return out


def step_bench():
    p = subprocess.run([sys.executable, os.path.join(args.tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"],
                       stdout=subprocess.PIPE, universal_newlines=True, cwd=args.tree)
    if p.returncode != 0:
        sys.exit(p.returncode)
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    return {"value": res.get("value"), "unit": res.get("unit"), "metric": res.get("metric")}


if not args.step:
    driver()
else:
    sys.path.insert(0, args.tree)
    res = {"update": step_update, "bench": step_bench}[args.step]()
    print(MARK + json.dumps(res), flush=True)
