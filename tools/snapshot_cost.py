#!/usr/bin/env python3
"""What a snapshot of a full-size handle costs (pcc_snapshot_bytes / pcc_snapshot / pcc_restore) next to a device-to-device copy of
the same number of bytes in the same process.  Two states: in lockstep after step 200 of an episode, and out of lockstep (episode
phases staggered as bench.py --stagger does) after 500 steps.  HIP events, 5 repeats after one warm-up, min - max; the bytes split
header / verbatim / rings.  pcc_snapshot_bytes is count + scan (and a stream synchronization: its host time is given too); what
pcc_snapshot adds to it is the header, the verbatim copies and the gather.
usage: snapshot_cost.py [n_envs] [out.json]"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import pcc_rl_amd
from pcc_rl_amd.env import _ptr

N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
OUT = sys.argv[2] if len(sys.argv) > 2 else None
REPEATS = 5
dev = torch.device("cuda:0")


def timed(fn):
    """(device ms, host ms) of fn(), events around it on the current stream."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record(); fn(); b.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return a.elapsed_time(b), host


def span(xs):
    return {"min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def measure(env, label):
    L, h, st = env._L, env._h, env._stream
    snap = env.snapshot()
    n = snap.nbytes
    head = snap.header()
    rings = 16 * head["ring_records"]
    buf, other = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    calls = {"pcc_snapshot_bytes": lambda: L.pcc_snapshot_bytes(h, st()),
             "pcc_snapshot": lambda: pcc_rl_amd.native.check(L.pcc_snapshot(h, _ptr(buf), n, st())),
             "pcc_restore": lambda: pcc_rl_amd.native.check(L.pcc_restore(h, _ptr(buf), n, st())),
             "memcpy_d2d_same_bytes": lambda: other.copy_(buf)}
    res = {"state": label, "n_envs": N, "bytes": {"total": n, "header": head["header_bytes"], "verbatim": n - rings - head["header_bytes"], "rings": rings},
           "ring_records": head["ring_records"], "records_per_sender": round(head["ring_records"] / (N * env.n_senders), 1)}
    for name, fn in calls.items():
        fn()   # warm-up
        runs = [timed(fn) for _ in range(REPEATS)]
        res[name] = dict(span([r[0] for r in runs]), host=span([r[1] for r in runs]))
    ref = res["memcpy_d2d_same_bytes"]["min_ms"]
    res["ratio_to_memcpy"] = {k: round(res[k]["min_ms"] / ref, 2) for k in ("pcc_snapshot_bytes", "pcc_snapshot", "pcc_restore")}
    env.check_flags()
    return res


env = pcc_rl_amd.BatchedNetworkEnv(N, device=dev, seed=0)
gen = torch.Generator(device=dev).manual_seed(1234)
acts = torch.rand((400, N), generator=gen, device=dev) * 2 - 1
env.reset()
for t in range(200):
    env.step(acts[t])
results = [measure(env, "lockstep, after step 200")]
env.reset()
phase = torch.arange(N, device=dev) % env.max_steps
for s in range(500):
    if 0 < s < env.max_steps:
        env.reset(phase == s)
    env.step(acts[s % 400])
results.append(measure(env, "out of lockstep (phases staggered), after 500 steps"))
results[-1]["restart_stats"] = env.restart_stats()
doc = {"tool": "tools/snapshot_cost.py", "device_bytes": env.device_bytes, "build": pcc_rl_amd.build.build_info(), "results": results}
text = json.dumps(doc, indent=1)
print(text)
if OUT:
    with open(OUT, "w") as f:
        f.write(text + "\n")
