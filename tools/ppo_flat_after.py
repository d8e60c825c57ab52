#!/usr/bin/env python3
"""What PPO and PopulationPPO hold after two iterate() calls from fixed seeds (1 024 envs, horizon 8), on every rollout, update
and checkpoint path they have (CASES), with the package of the tree this file sits in, into a .pt file -- to hold two trees
against each other (GPU box):
   python tools/ppo_flat_after.py out.pt            in each tree (also writes out.pt.ckpt: the state_dict() of CKPT_CASES), then
   python tools/ppo_flat_after.py --compare a.pt b.pt        torch.equal on every tensor, == on every key list
   python tools/ppo_flat_after.py --resume other.pt.ckpt cross.pt     the OTHER tree's checkpoints loaded here, one more iterate()
   python tools/ppo_flat_after.py --compare-subset cross.pt other.pt  ... against the other tree's own continuation
Per case: the parameters, Adam's moments, the observation, the normaliser and the hyper rows where they exist, the mean rewards;
sorted(state_dict().keys()); and all tensors again after one more iterate() of the agent itself ("continued") and of a freshly
built twin that loaded its state_dict() ("resumed").  Uses only keywords every tree since normalize_obs has: a tree that
restructures the trainers must leave every entry as it was."""
import io, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

N, T, DEV, POOLS = 1024, 8, "cuda:0", (2, 8, 32)
SEEDS = [3, 4, 5, 6]


def cases():
    import pcc_rl_amd
    from pcc_rl_amd.ppo import PPO, PopulationPPO
    one = lambda: pcc_rl_amd.BatchedNetworkEnv(N, device=DEV, seed=11, ring_pools=POOLS)
    two = lambda: pcc_rl_amd.GroupedNetworkEnv(N, 2, device=DEV, seed=11, ring_pools=POOLS)
    ppo = lambda **kw: (lambda env: PPO(env, horizon=T, seed=3, **kw))
    pop = lambda **kw: (lambda env: PopulationPPO(env, 4, horizon=T, seeds=SEEDS, **kw))
    # name: (env, agent, evolve(scores = the first iteration's mean rewards, seed=1) between the two iterations?)
    return {"ppo": (one, ppo(), False), "population": (one, pop(), False),
            "ppo_in_step": (one, ppo(policy_in_step=True), False),
            "ppo_groups": (two, ppo(), False), "ppo_groups_in_step": (two, ppo(policy_in_step=True), False),
            "ppo_norm": (one, ppo(normalize_obs=True), False),
            "ppo_arch3": (one, ppo(arch=(32, 16, 8)), False),            # the framework rollout and the framework update
            "ppo_framework_update": (one, ppo(fused_update=False), False),
            "population_norm": (one, pop(normalize_obs=True), False), "population_evolve": (one, pop(), True)}


CKPT_CASES = ("ppo", "population_norm")   # their state_dict()s go into <out>.ckpt for the other tree's --resume


def put(res, prefix, agent, rewards):
    t = {"obs": agent.obs, "rewards": torch.tensor(rewards, dtype=torch.float64)}
    if hasattr(agent, "flat"):
        t.update(flat=agent.flat, adam_m=agent.adam_m, adam_v=agent.adam_v)
    else:   # PPO's framework update: the module's parameters and torch.optim.Adam's moments
        t["flat"] = agent.policy.flat_params()
        for i, st in enumerate(agent.opt.state_dict()["state"].values()):
            t["adam_m%d" % i], t["adam_v%d" % i] = st["exp_avg"], st["exp_avg_sq"]
    if getattr(agent, "normalize_obs", False):
        t.update(raw_obs=agent.raw_obs, norm_stats=agent.obs_norm.stats, norm_norm=agent.obs_norm.norm)
    if hasattr(agent, "hyper"):
        t["hyper"] = agent.hyper
    torch.cuda.synchronize()
    res.update({prefix + "/" + k: v.detach().cpu().clone() for k, v in t.items()})


def dump(out):
    res, ckpt = {}, {}
    for name, (make_env, make_agent, evolve) in cases().items():
        env = make_env()
        agent = make_agent(env)
        rewards = []
        for i in range(2):
            rewards.append(agent.iterate()["mean_step_reward"])
            if evolve and i == 0:
                agent.evolve(scores=rewards[0], seed=1)
        put(res, name, agent, rewards)
        f = io.BytesIO()
        torch.save(agent.state_dict(), f)   # (as a checkpoint is kept: torch.optim.Adam's state_dict shares its tensors with the optimiser)
        f.seek(0)
        sd = torch.load(f)
        res[name + "/state_dict_keys"] = sorted(sd.keys())
        if name in CKPT_CASES:
            ckpt[name] = sd
        put(res, name + "/continued", agent, [agent.iterate()["mean_step_reward"]])
        env2 = make_env()
        twin = make_agent(env2)   # (reseeds torch's generators: load_state_dict puts them back)
        twin.load_state_dict(sd)
        put(res, name + "/resumed", twin, [twin.iterate()["mean_step_reward"]])
        same = all(torch.equal(res[k], res[k.replace("/continued/", "/resumed/")]) for k in res if k.startswith(name + "/continued/"))
        print(name, "resumed == continued" if same else "resumed DIFFERS from continued", flush=True)
        env.close(); env2.close()
    torch.save(res, out)
    torch.save(ckpt, out + ".ckpt")
    print("wrote", out, len(res), "entries;", out + ".ckpt", sorted(ckpt))


def resume(ckpt, out):
    res, all_cases = {}, cases()
    for name, sd in torch.load(ckpt).items():
        make_env, make_agent, _ = all_cases[name]
        env = make_env()
        agent = make_agent(env)
        agent.load_state_dict(sd)
        put(res, name + "/resumed", agent, [agent.iterate()["mean_step_reward"]])
        env.close()
    torch.save(res, out)
    print("wrote", out, len(res), "entries")


def compare(a, b, subset=False):
    A, B = torch.load(a), torch.load(b)
    assert set(A) <= set(B) if subset else sorted(A) == sorted(B)
    same = lambda x, y: torch.equal(x, y) if torch.is_tensor(x) else x == y
    bad = [k for k in sorted(A) if not same(A[k], B[k])]
    for k in sorted(A):
        print(k, "equal" if k not in bad else "DIFFERENT")
    print("%d entries, %d different" % (len(A), len(bad)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if sys.argv[1] in ("--compare", "--compare-subset"):
        compare(sys.argv[2], sys.argv[3], subset=sys.argv[1] == "--compare-subset")
    elif sys.argv[1] == "--resume":
        resume(sys.argv[2], sys.argv[3])
    else:
        dump(sys.argv[1])
