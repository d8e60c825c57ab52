#!/usr/bin/env python3
"""What the update diagnostics and the KL guard cost (GPU box only).  A driver and its steps: the driver starts
every step as a fresh process under a time limit of its own, one after the other, stops at the first step that fails and merges what
the steps printed into --out.  The steps --
  kernels        the library's calls alone on one rollout's rows, [--horizon][envs] at every --envs size, --members count and
                 --row-steps value: the forward of the selected rows (pcc_policy_act_rows_pop), the walk + merge (pcc_update_diag_pop)
                 and a whole check (both).  Windows of --inner calls, --repeats repeats after a warm-up, the variants alternating.
  iterate_off    PPO.iterate() and PopulationPPO.iterate() (K = --population) with default options in the tree --tree: three windows
                 of --iterate-inner calls.  With --parent the driver runs this step --repeats times in this tree and in the parent's,
                 alternating, and compares window by window: this tree's median against the parent's min - max.
  iterate_on     both trainers without the options, with diagnostics and with --target-kl, alternating in one process; and the same
                 with lr = 0 (the same launches on the same kind of trajectories: the difference is the options' own work)
  bench          bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline in --tree (the driver: --repeats runs per tree, alternating)
Microseconds (kernels) or milliseconds (iterate) per call, host clock around a device synchronise.
   python tools/update_diag_cost.py [--out profiles/r24_update_diag.json] [--parent DIR] [--skip bench,iterate_on]"""
import argparse, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_update_diag.json"))
ap.add_argument("--step", default="", choices=("", "kernels", "iterate_off", "iterate_on", "bench"))
ap.add_argument("--tree", default=ROOT, help="the source tree a step imports the package from (with its own built library)")
ap.add_argument("--parent", default="", help="a checkout of the parent commit with its own built library: iterate_off and bench run there too")
ap.add_argument("--parent-first", action="store_true", help="the parent's process first in every alternating pair (default: this tree's)")
ap.add_argument("--skip", default="", help="steps the driver leaves out, comma-separated")
ap.add_argument("--envs", default="65536,262144")
ap.add_argument("--horizon", type=int, default=64)
ap.add_argument("--members", default="1,8,32")
ap.add_argument("--row-steps", default="1,8")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--inner", type=int, default=10, help="calls per timed window of the kernels step")
ap.add_argument("--iterate-envs", type=int, default=65536)
ap.add_argument("--population", type=int, default=4)
ap.add_argument("--iterate-inner", type=int, default=2, help="iterate() calls per timed window")
ap.add_argument("--target-kl", type=float, default=0.02)
ap.add_argument("--step-timeout", type=int, default=240, help="seconds a step may take")
args = ap.parse_args()
T = args.horizon
MARK = "RESULT_JSON "


def driver():
    skip = set(x for x in args.skip.split(",") if x)
    out = {"what": "tools/update_diag_cost.py: every step a fresh process under `timeout`, chained; see the tool's docstring",
           "horizon": T, "repeats": args.repeats}
    common = ["--horizon", str(T), "--repeats", str(args.repeats), "--inner", str(args.inner), "--iterate-envs", str(args.iterate_envs),
              "--population", str(args.population), "--iterate-inner", str(args.iterate_inner), "--target-kl", str(args.target_kl),
              "--envs", args.envs, "--members", args.members, "--row-steps", args.row_steps]

    def run(step, tree):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--tree", tree] + common
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, cwd=tree)
        sys.stdout.write(p.stdout[-3000:])
        if p.returncode != 0:   # a fault, an abort or the time limit: nothing more is started on the GPU
            print("step %s in %s ended with status %d: stopping here" % (step, tree, p.returncode), flush=True)
            save(out)
            sys.exit(1)
        return json.loads([l for l in p.stdout.splitlines() if l.startswith(MARK)][-1][len(MARK):])

    trees = [("this_tree", ROOT)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    if args.parent_first:
        trees.reverse()
    if "kernels" not in skip:
        out["kernels"] = run("kernels", ROOT)
    if "iterate_off" not in skip:
        runs = {name: [] for name, _ in trees}
        for _ in range(args.repeats):
            for name, tree in trees:
                runs[name].append(run("iterate_off", tree))
        out["iterate_options_off"] = compare_windows(runs)
    if "iterate_on" not in skip:
        out["iterate_options_on"] = run("iterate_on", ROOT)
    if "bench" not in skip:
        runs = {name: [] for name, _ in trees}
        for _ in range(args.repeats):
            for name, tree in trees:
                runs[name].append(run("bench", tree))
        out["bench"] = {name: {"value": [r["value"] for r in rs], "unit": rs[0].get("unit")} for name, rs in runs.items()}
        if "parent" in runs:
            mine, theirs = sorted(out["bench"]["this_tree"]["value"]), out["bench"]["parent"]["value"]
            out["bench"]["median_inside_parent_min_max"] = bool(min(theirs) <= mine[len(mine) // 2] <= max(theirs))
    save(out)


def compare_windows(runs):
    """{trainer: {window: {tree: [ms per process], ...}}} and, with a parent, whether this tree's median lies inside its min - max."""
    out = {}
    for trainer in runs["this_tree"][0]:
        rows = []
        for w in range(len(runs["this_tree"][0][trainer])):
            row = {name: [r[trainer][w] for r in rs] for name, rs in runs.items()}
            if "parent" in row:
                med = sorted(row["this_tree"])[len(row["this_tree"]) // 2]
                row["this_tree_median"] = med
                row["inside_parent_min_max"] = bool(min(row["parent"]) <= med <= max(row["parent"]))
                row["below_parent_min"] = bool(med < min(row["parent"]))
            rows.append(row)
        out[trainer] = rows
    return out


def save(out):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


def timed(fn, inner, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def alternate(variants, torch, scale):
    """{name: [time per repeat]} of {name: (fn, inner)}: a warm-up window of every variant, then the repeats, the variants alternating"""
    times = {name: [] for name in variants}
    for rep in range(-1, args.repeats):
        for name, (fn, inner) in variants.items():
            t = timed(fn, inner, torch) * scale
            if rep >= 0:
                times[name].append(t)
    return times


def step_kernels():
    import torch
    from pcc_rl_amd import build as pbuild
    from pcc_rl_amd.env import _ptr
    from pcc_rl_amd.native import call, current_stream
    from pcc_rl_amd.updiag import UpdateDiagnostics
    dev = torch.device("cuda:0")
    D, arch = 30, (32, 16)
    n_params = 2 * (arch[0] * D + arch[0] + arch[1] * arch[0] + 2 * arch[1] + 1) + 1
    stride = (n_params + 63) // 64 * 64
    out = {"device": torch.cuda.get_device_name(0), "build": pbuild.build_info(), "unit": "microseconds per call", "inner": args.inner,
           "obs_dim": D, "arch": list(arch)}
    g = torch.Generator(device=dev).manual_seed(1)
    for N in [int(x) for x in args.envs.split(",")]:
        obs = torch.randn((T, N, D), device=dev, generator=g)
        act, logp, ret, val = (torch.randn((T, N), device=dev, generator=g) for _ in range(4))
        for K in [int(x) for x in args.members.split(",")]:
            flat = 0.1 * torch.randn((K, stride), device=dev, generator=g)
            hyper = torch.tensor([[1e-3, 0.2, 0.01, 0.99, 0.95, 0, 0, 0]] * K, dtype=torch.float32, device=dev)
            for rs in [int(x) for x in args.row_steps.split(",")]:
                ud = UpdateDiagnostics(N, K, dev, rs)
                ud.begin(hyper)
                check = lambda: ud.check(1, obs, act, logp, ret, val, flat, stride, n_params, arch, hyper, 0.03)
                check()
                stream = current_stream(dev)
                forward = lambda: call("pcc_policy_act_rows_pop", _ptr(obs), T, rs, N, D, _ptr(flat), stride, K, arch[0], arch[1],
                                       _ptr(ud.mean_new), None, stream)
                walk = lambda: call("pcc_update_diag_pop", _ptr(act), _ptr(logp), _ptr(ud.mean_new), _ptr(ret), _ptr(val), T, rs, N, K, _ptr(flat),
                                    stride, (n_params - 1) // 2, _ptr(hyper), 0.03, 1, _ptr(ud.diag), 8, _ptr(ud.stop), _ptr(ud.hyper_live),
                                    _ptr(ud._scratch), stream)
                times = alternate({"forward": (forward, args.inner), "walk_and_merge": (walk, args.inner), "check": (check, args.inner)}, torch, 1e6)
                rows = (T - 1) // rs + 1
                row = {name + "_us": t for name, t in times.items()}
                row.update({name + "_us_min_max": [min(t), max(t)] for name, t in times.items()})
                row["rows"], row["walk_bytes"] = rows, rows * N * 20
                row["walk_gb_per_s_of_min"] = row["walk_bytes"] / (min(times["walk_and_merge"]) * 1e-6) / 1e9
                out["envs_%d_members_%d_row_step_%d" % (N, K, rs)] = row
                print("envs = %d, members = %d, row_step = %d: %s" % (N, K, rs, json.dumps(row)), flush=True)
                del ud
        del obs, act, logp, ret, val
        torch.cuda.empty_cache()
    return out


def trainer(kind, pcc_rl_amd, PPO, PopulationPPO, lr=1e-3, **kw):
    """(env, agent): the tools/ppo_throughput.py shapes; kind "ppo" or "population_k<K>"."""
    N, K = args.iterate_envs, args.population
    env = pcc_rl_amd.BatchedNetworkEnv(N, device="cuda:0", seed=0, ring_pools=(1, 2, 8))
    if kind == "ppo":
        return env, PPO(env, horizon=T, seed=0, minibatch=max(2048, N * T // 4), lr=lr, **kw)
    return env, PopulationPPO(env, K, horizon=T, lr=lr, **kw)


def step_iterate_off():
    """Default options, three windows after a warm-up window: three phases of the episode, compared window by window."""
    import torch
    import pcc_rl_amd
    from pcc_rl_amd.ppo import PPO, PopulationPPO
    out = {}
    for kind in ("ppo", "population_k%d" % args.population):
        env, agent = trainer(kind, pcc_rl_amd, PPO, PopulationPPO)
        out[kind] = [timed(agent.iterate, args.iterate_inner, torch) * 1e3 for _ in range(4)][1:]
        env.check_flags()
        env.close()
        del agent, env
        torch.cuda.empty_cache()
    return out


def step_iterate_on():
    import torch
    import pcc_rl_amd
    from pcc_rl_amd.ppo import PPO, PopulationPPO
    out = {"unit": "milliseconds per iterate()", "target_kl": args.target_kl}
    options = {"off": {}, "diagnostics": {"diagnostics": True}, "diagnostics_rows_8": {"diagnostics": True, "diag_rows": 8},
               "target_kl": {"target_kl": args.target_kl}}
    for label, lr in (("training", 1e-3), ("frozen_lr_0", 0.0)):
        for kind in ("ppo", "population_k%d" % args.population):
            made = {name: trainer(kind, pcc_rl_amd, PPO, PopulationPPO, lr=lr, **kw) for name, kw in options.items()}
            times = alternate({name: (m[1].iterate, args.iterate_inner) for name, m in made.items()}, torch, 1e3)
            row = {name + "_ms": t for name, t in times.items()}
            for name in times:
                if name != "off":
                    row[name + "_added_ms_of_min"] = min(times[name]) - min(times["off"])
            out["%s_%s" % (kind, label)] = row
            print("%s %s: %s" % (kind, label, json.dumps(row)), flush=True)
            for env, _ in made.values():
                env.check_flags()
                env.close()
            del made
            torch.cuda.empty_cache()
    return out


def step_bench():
    p = subprocess.run([sys.executable, os.path.join(args.tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"], stdout=subprocess.PIPE,
                       universal_newlines=True, cwd=args.tree)
    if p.returncode != 0:
        sys.exit(p.returncode)
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    return {"value": res.get("value"), "unit": res.get("unit"), "metric": res.get("metric")}


if not args.step:
    driver()
else:
    sys.path.insert(0, args.tree)
    res = {"kernels": step_kernels, "iterate_off": step_iterate_off, "iterate_on": step_iterate_on, "bench": step_bench}[args.step]()
    print(MARK + json.dumps(res), flush=True)
