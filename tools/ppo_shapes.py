#!/usr/bin/env python3
"""The fused PPO update and policy forward against the framework paths they replace, per policy shape (GPU box only).
For each (observation length; h1, h2): `update_s` of PPO.update fused and with fused_update=False on the same rollout, and
`t_roll` of PPO.collect with the library forward (pcc_policy_act) and with the framework forward (MlpPolicy.act + env.step);
the two variants alternate inside one process, each repeated --reps times after a warm-up of every shape; times are a host
clock around work that ends in a device synchronise.
   python tools/ppo_shapes.py [--envs 65536] [--horizon 64] [--reps 3] [--shapes 30:32,16 36:32,16 60:64,32 120:64,64] [--out f.json]
   python tools/ppo_shapes.py --kernels 120:64,64     a few fused updates + rollout steps of one shape and nothing else: the
                                                      run to put under `rocprofv3 --kernel-trace --stats -- python ...`
Observation lengths are history x features: 30 = 10 x the 3 default features, otherwise history (length / 12) x all 12."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import pcc_rl_amd
from pcc_rl_amd.ppo import PPO

PEAK_FP32_MATRIX = 157.3e12   # MI355X, fp32 MFMA, FLOP/s


def parse_shape(text):
    d, arch = text.split(":")
    return int(d), tuple(int(x) for x in arch.split(","))


def make_env(n, D, seed=0):
    if D == 30:
        return pcc_rl_amd.BatchedNetworkEnv(n, device="cuda:0", seed=seed)
    if D % 12:
        raise SystemExit("observation length %d: 30 or a multiple of 12" % D)
    return pcc_rl_amd.BatchedNetworkEnv(n, device="cuda:0", seed=seed, history_len=D // 12, features=list(pcc_rl_amd.METRIC_NAMES))


def grad_flops(D, arch, samples):
    """Forward + the two backward contractions (dW, dh) of both networks: 3 x 2 FLOP per weight and sample."""
    h1, h2 = arch
    return 2 * 6 * (D * h1 + h1 * h2 + h2) * samples


def once(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", nargs="+", default=["30:32,16", "36:32,16", "60:64,32", "120:64,64"])
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, T = a.envs, a.horizon
    mb = max(2048, N * T // 4)
    if a.kernels:
        D, arch = parse_shape(a.kernels)
        env = make_env(N, D)
        agent = PPO(env, arch=arch, horizon=T, seed=0, minibatch=mb)
        assert agent.fused_update
        batch = agent.collect()
        for _ in range(2):
            agent.update(*batch[:5])
        torch.cuda.synchronize()
        env.close()
        return
    from pcc_rl_amd import build as pbuild
    out = {"n_envs": N, "horizon": T, "minibatch": mb, "reps": a.reps, "library": pbuild.build_info(), "shapes": []}
    runs = []
    for text in a.shapes:
        D, arch = parse_shape(text)
        env = make_env(N, D)
        fused = PPO(env, arch=arch, horizon=T, seed=0, minibatch=mb)
        fw = PPO(env, arch=arch, horizon=T, seed=0, minibatch=mb, fused_update=False)
        fw.policy.fused_ok = lambda obs: False   # the framework forward: MlpPolicy.act + env.step per step
        assert fused.fused_update, text
        batch = fused.collect()
        runs.append((text, D, arch, env, fused, fw, batch))
        # warm-up of every variant of this shape
        fused.update(*batch[:5]); fw.update(*batch[:5]); fused.collect(); fw.collect()
        torch.cuda.synchronize()
    for text, D, arch, env, fused, fw, batch in runs:
        t = {"update_fused_s": [], "update_framework_s": [], "t_roll_library_s": [], "t_roll_framework_s": []}
        for _ in range(a.reps):   # alternating
            t["update_fused_s"].append(once(lambda: fused.update(*batch[:5])))
            t["update_framework_s"].append(once(lambda: fw.update(*batch[:5])))
            t["t_roll_library_s"].append(once(fused.collect))
            t["t_roll_framework_s"].append(once(fw.collect))
        steps = fused.epochs * ((N * T + mb - 1) // mb)
        fl = grad_flops(D, arch, N * T * fused.epochs)
        best = min(t["update_fused_s"])
        out["shapes"].append({"obs_dim": D, "arch": list(arch), "optimiser_steps_per_update": steps, **t,
                              "grad_flop_per_update": fl,
                              "update_fused_share_of_fp32_matrix_peak": fl / best / PEAK_FP32_MATRIX,
                              "note": "share of peak from the whole update's best host time (gradient + Adam + launches), not a kernel time"})
        env.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
