#!/usr/bin/env python3
"""Which kernels the host side launches, in which order, with which grids: a short scenario over the step paths of
pcc_sim.hip, to be traced once per library (PCC_SIM_LIBRARY selects another build of libpcc_sim.so) and compared.

    rocprofv3 --kernel-trace --output-format csv -d DIR_A -- python tools/launch_sequence.py
    PCC_SIM_LIBRARY=other/libpcc_sim.so rocprofv3 --kernel-trace --output-format csv -d DIR_B -- python tools/launch_sequence.py
    python tools/launch_sequence.py compare DIR_A DIR_B [report.txt]

The scenario (episodes of 5 steps, so every part crosses episode boundaries): 64 envs with the defaults -- step, step_many,
rollout; 256 envs with work lists, 1 and 8 partitions -- step in lockstep, step after a masked reset (restart list, then
shadows), step_send / step_retire, the one-launch step, rollout with the retire-launch epilogue; 256 envs with latency noise;
256 envs with the congestion window (without and with lists); 8 192 envs with the defaults.
`compare` holds the two traces against each other: the dispatches in host order (Dispatch_Id) and queue by queue, each as
(kernel, grid, workgroup size); exit status 1 when they differ."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scenario():
    import torch
    import pcc_rl_amd
    from pcc_rl_amd.ppo import MlpPolicy

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)

    def actions(*shape):
        return torch.rand(shape, generator=gen, device=dev) * 2 - 1

    def make(n, knobs=None, **kw):
        env = pcc_rl_amd.BatchedNetworkEnv(n, device=dev, seed=3, max_steps=5, **kw)
        env.set_tuning(**(knobs or {}))
        env.reset()
        return env

    def steps(env, k, width=1):
        for _ in range(k):
            env.step(actions(env.n_envs, width))

    def rollout(env, T):
        torch.manual_seed(1)
        params = MlpPolicy(env.obs_dim, 1, (32, 16)).flat_params().to(dev)
        N, S = env.n_envs, env.n_senders
        obs = torch.zeros((T + 1, N, S, env.obs_dim), device=dev)
        obs[0].copy_(env._obs)
        out = [torch.zeros((T, N, S), device=dev) for _ in range(4)]
        env.rollout(params, torch.randn((T, N, S), generator=gen, device=dev), obs, out[0], out[1], out[2], out[3],
                    torch.zeros((T, N), dtype=torch.uint8, device=dev))

    def finish(env):
        torch.cuda.synchronize()
        env.check_flags()
        env.close()

    env = make(64)
    steps(env, 7)
    env.step_many(actions(12, 64), obs_out=torch.zeros((12, 64, 1, env.obs_dim), device=dev))
    rollout(env, 12)
    finish(env)

    for parts in (1, 8):
        env = make(256, dict(list_min_envs=0, parts=parts))
        steps(env, 7)
        env.reset(torch.arange(256, device=dev) % 3 == 0)     # out of lockstep: the restart list, then shadows
        steps(env, 12)
        for _ in range(6):
            env.step_send(actions(256, 1))
            env.step_retire()
        rollout(env, 8)
        env.set_tuning(fused=1)
        env.reset()
        steps(env, 7)
        assert env.fused_steps() > 0
        env.set_tuning(fused=0, rollout_epilogue=1)
        env.reset()
        rollout(env, 12)
        env.reset(torch.arange(256, device=dev) % 3 == 0)
        rollout(env, 8)
        finish(env)

    env = make(256, latency_noise=1.1)
    steps(env, 7)
    finish(env)

    for knobs in (None, dict(list_min_envs=0)):
        env = make(256, knobs, use_cwnd=True)
        steps(env, 7, width=2)
        finish(env)

    env = make(8192, ring_pools=(2, 8, 32))
    steps(env, 7)
    finish(env)


def dispatches(directory):
    """[(queue, kernel, grid, workgroup)] of a trace directory in host order, the queues numbered as they first appear."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    size = lambda r, what: tuple(int(r[what + "_" + axis]) for axis in "XYZ")
    queues = {}
    return [(queues.setdefault(r.get("Queue_Id"), len(queues)), r["Kernel_Name"], size(r, "Grid_Size"), size(r, "Workgroup_Size"))
            for r in rows]


def compare(dir_a, dir_b, report=None):
    a, b = dispatches(dir_a), dispatches(dir_b)
    lines = ["%s: %d dispatches on %d queues" % (d, len(x), len({q for q, _, _, _ in x})) for d, x in ((dir_a, a), (dir_b, b))]
    same = bool(a) and len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if x[1:] != y[1:]:
            same = False
            lines.append("host order differs first at dispatch %d:\n  %r\n  %r" % (i, x, y))
            break
    for q in sorted({q for q, _, _, _ in a + b}):
        qa, qb = [x[1:] for x in a if x[0] == q], [y[1:] for y in b if y[0] == q]
        if qa != qb:
            same = False
            first = next((i for i, (x, y) in enumerate(zip(qa, qb)) if x != y), min(len(qa), len(qb)))
            lines.append("queue %d differs first at its dispatch %d (%d against %d dispatches)" % (q, first, len(qa), len(qb)))
    names = {}
    for _, name, _, _ in a:
        short = name.split("(")[0].replace("void ", "").replace("(anonymous namespace)::", "")
        names[short] = names.get(short, 0) + 1
    lines.append("kernels of the first trace: " + ", ".join("%s x %d" % kv for kv in sorted(names.items())))
    lines.append("verdict: " + ("IDENTICAL -- the same (kernel, grid, workgroup size) in host order and on every queue" if same
                                else "DIFFERENT"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if report:
        with open(report, "w") as f:
            f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:5]))
    scenario()
