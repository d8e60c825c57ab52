"""Population PPO, the part that needs no GPU: the three C-ABI symbols (include/pcc_policy.h: pcc_policy_act_pop,
pcc_ppo_minibatch_step_pop, pcc_gae_pop), the compiler's resource report of the kernels they share with the stand-alone calls, the sample-index helper and
the permutations, the per-member advantage normalisation, and what PopulationPPO's constructor refuses."""
import json

import pytest
import torch

from pcc_rl_amd import native
from pcc_rl_amd.native import lib
from pcc_rl_amd.ppo import PopulationPPO, normalise_per_member, population_permutations, population_sample_index

POP_SYMBOLS = ("pcc_policy_act_pop", "pcc_ppo_minibatch_step_pop", "pcc_gae_pop")
FIXED, MFMA = (3, 6, 12, 30, 36, 60), (3, 6, 12, 30)   # PCC_FIXED_OBS_LENGTHS / PCC_MFMA_OBS_LENGTHS of csrc/pcc_policy_dev.h


def test_the_three_symbols_are_exported():
    L = lib()
    for s in POP_SYMBOLS:
        assert s in native.SYMBOLS, s
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
    assert len(L.pcc_policy_act_pop.argtypes) == 14 and len(L.pcc_ppo_minibatch_step_pop.argtypes) == 26
    assert len(L.pcc_gae_pop.argtypes) == 11


def test_population_kernels_use_no_scratch(tmp_path):
    """A build into a temporary file: every PPO-stage kernel -- one per stage, its grid with a member dimension, serving the
    stand-alone and the population entry points alike -- is in the compiler's resource report with 0 bytes of scratch and 0 spilled
    vector registers, at the figures tests/test_ppo_shapes.py pins; no population twin and no copied body is left."""
    from pcc_rl_amd import build as pbuild
    out = str(tmp_path / "libpcc_sim_pop.so")
    pbuild.build_library(force=True, out=out)
    res = json.load(open(out + ".resources.json"))
    names = ["ppo_adam_kernel", "gae_kernel"]
    names += ["policy_act_fixed_kernel<%d, 32, 16>" % D for D in FIXED] + ["policy_act_kernel<%d>" % D for D in FIXED]
    names += ["ppo_grad_mfma_kernel<%d, 32, 16>" % D for D in MFMA]
    for kern in ("ppo_grad_tiled_kernel", "policy_act_tiled_kernel"):
        names += ["pcc_tiles::%s<%d, %d, %d>" % (kern, D, h1, h2) for D in (32, 64, 128) for h1, h2 in ((32, 32), (64, 32), (64, 64))]
    for name in names:
        assert name in res, name
        assert res[name]["scratch"] == 0 and res[name]["vgpr_spills"] == 0, (name, res[name])
        assert res[name]["lds"] <= 160 * 1024, (name, res[name])
    assert not [n for n in res if "_pop_kernel" in n or "_body" in n]
    stages = ("ppo_adam", "gae_", "policy_act", "ppo_grad")   # no PPO-stage kernel goes unchecked
    assert sorted(n for n in res if any(s in n for s in stages)) == sorted(names)
    assert (res["ppo_grad_mfma_kernel<30, 32, 16>"]["vgprs"], res["ppo_grad_mfma_kernel<30, 32, 16>"]["lds"]) == (256, 52736)
    assert res["policy_act_fixed_kernel<30, 32, 16>"]["vgprs"] == 87


def test_sample_index_and_permutations():
    T, N, K = 5, 12, 3
    n_m = N // K
    flat = torch.arange(T * N).reshape(T, N)
    for m in range(K):
        for t in range(T):
            for e in range(n_m):
                assert population_sample_index(m, t, e, N, K) == int(flat[t, m * n_m + e])
    # tensors too
    t, e = torch.meshgrid(torch.arange(T), torch.arange(n_m), indexing="ij")
    assert torch.equal(population_sample_index(1, t, e, N, K), flat[:, n_m:2 * n_m])
    g = torch.Generator().manual_seed(4)
    perm = population_permutations(T, N, K, generator=g)
    assert perm.shape == (K, T * n_m) and perm.dtype == torch.int64 and perm.is_contiguous()
    for m in range(K):
        own = flat[:, m * n_m:(m + 1) * n_m].reshape(-1)
        assert torch.equal(perm[m].sort().values, own.sort().values)     # exactly its own samples, each once
        assert not torch.equal(perm[m], own)                              # ... shuffled
    again = population_permutations(T, N, K, generator=g)
    assert not torch.equal(again, perm)                                   # a new draw per call (per epoch)
    # an odd member size, one member
    perm = population_permutations(7, 257, 1, generator=g)
    assert torch.equal(perm[0].sort().values, torch.arange(7 * 257))


def test_normalise_equals_a_per_member_loop():
    T, K, n_m = 6, 3, 37
    g = torch.Generator().manual_seed(2)
    adv = torch.randn(T, K * n_m, generator=g) * torch.tensor([1.0, 10.0, 0.1]).repeat_interleave(n_m) + 3.0
    got = normalise_per_member(adv, K)
    for m in range(K):
        a = adv[:, m * n_m:(m + 1) * n_m].contiguous().reshape(-1)
        want = ((a - a.mean()) / (a.std() + 1e-8)).reshape(T, n_m)
        assert torch.equal(got[:, m * n_m:(m + 1) * n_m], want)
        assert abs(float(want.mean())) < 1e-5 and abs(float(want.std()) - 1.0) < 1e-5
    assert got.shape == adv.shape


class _Env(object):   # what the constructor's argument checks look at, without a simulator behind it
    obs_dim, device, n_senders, n_envs = 30, "cuda:0", 1, 12


def test_constructor_refuses():
    with pytest.raises(ValueError, match="do not divide"):
        PopulationPPO(_Env(), 5)
    with pytest.raises(ValueError, match="two hidden layers"):
        PopulationPPO(_Env(), 3, arch=(32, 16, 8))
    for kw in ({"lr": [1e-3, 1e-4]}, {"clip": [0.2] * 4}, {"ent_coef": []}, {"gamma": [0.99, 0.9]}, {"lam": [0.95] * 5}, {"seeds": [0, 1]}):
        with pytest.raises(ValueError, match="%s has %d values for 3 members" % (list(kw)[0], len(list(kw.values())[0]))):
            PopulationPPO(_Env(), 3, **kw)
    import numpy as np
    with pytest.raises(ValueError, match="lr has 2 values"):         # a tensor or an array is a sequence ...
        PopulationPPO(_Env(), 3, lr=torch.tensor([1e-3, 1e-4]))
    with pytest.raises(ValueError, match="gamma has 4 values"):
        PopulationPPO(_Env(), 3, gamma=np.array([0.9, 0.99, 0.95, 0.999]))
    with pytest.raises(ValueError, match="BatchedNetworkEnv"):       # ... a numpy scalar or a 0-dim tensor a scalar: past the argument checks
        PopulationPPO(_Env(), 3, lr=np.float32(1e-3), clip=torch.tensor(0.2))
    with pytest.raises(ValueError, match="members = 0"):
        PopulationPPO(_Env(), 0)
    with pytest.raises(ValueError, match="BatchedNetworkEnv"):   # valid arguments, but not an env of the library (no framework path)
        PopulationPPO(_Env(), 3, lr=[1e-3, 3e-4, 0.0])
