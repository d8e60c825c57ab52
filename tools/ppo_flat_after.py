#!/usr/bin/env python3
"""PPO's and PopulationPPO's parameters and Adam state after two iterate() calls from fixed seeds (1 024 envs, horizon 8, default
keywords), with the package of the tree this file sits in, into a .pt file -- to hold two trees against each other (GPU box):
   python tools/ppo_flat_after.py out.pt            in each tree, then
   python tools/ppo_flat_after.py --compare a.pt b.pt        torch.equal on every tensor
Uses only keywords every tree since PopulationPPO has: a tree that adds an opt-in keyword must leave these tensors as they were
(normalize_obs=False against the tree before it)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def dump(out):
    import pcc_rl_amd
    from pcc_rl_amd.ppo import PPO, PopulationPPO
    res = {}
    for name, make in (("ppo", lambda env: PPO(env, horizon=8, seed=3)), ("population", lambda env: PopulationPPO(env, 4, horizon=8, seeds=[3, 4, 5, 6]))):
        env = pcc_rl_amd.BatchedNetworkEnv(1024, device="cuda:0", seed=11, ring_pools=(2, 8, 32))
        agent = make(env)
        rewards = [agent.iterate()["mean_step_reward"] for _ in range(2)]
        torch.cuda.synchronize()
        res.update({name + "/flat": agent.flat.cpu(), name + "/adam_m": agent.adam_m.cpu(), name + "/adam_v": agent.adam_v.cpu(),
                    name + "/obs": agent.obs.cpu(), name + "/rewards": torch.tensor(rewards, dtype=torch.float64)})
        env.close()
    torch.save(res, out)
    print("wrote", out, len(res), "tensors")


def compare(a, b):
    A, B = torch.load(a), torch.load(b)
    assert sorted(A) == sorted(B)
    bad = [k for k in sorted(A) if not torch.equal(A[k], B[k])]
    for k in sorted(A):
        print(k, "equal" if k not in bad else "DIFFERENT")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        dump(sys.argv[1])
