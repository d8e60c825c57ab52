"""Population-based training's step between generations on the GPU (include/pcc_policy.h: pcc_pbt_evolve;
pcc_rl_amd.ppo.PopulationPPO.evolve).  Every comparison is torch.equal, the float blocks as int32 views so that NaN payloads
and signed zeros count; the reference is evolve_reference of tests/test_pbt_cpu.py, a numpy restatement of the header's contract
with its own Philox and an explicit O(K^2) ranking.  Shapes: the smallest that can go wrong -- one member, odd member counts, a
float4 tail, one float per row, rows over 25 workgroups, the member limit."""
import ctypes

import numpy as np
import pytest
import torch

import pcc_rl_amd
from pcc_rl_amd.native import lib
from pcc_rl_amd.ppo import PopulationPPO, explore_matrix, population_permutations

from test_pbt_cpu import DRAWS, EXPLORE, PAD, SCORE_KINDS, SHAPES, evolve_reference, make_case, make_scores, n_cuts

DEV = "cuda:0"
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _evolve(score, n_cut, blocks, n_params, seed, generation, outs=(True, True)):
    """pcc_pbt_evolve on device copies of the numpy inputs; returns the six device tensors (an output that was not asked for: None)."""
    K = len(score)
    P, M, V, H = (torch.from_numpy(b.copy()).to(DEV) for b in blocks)
    s = torch.from_numpy(np.asarray(score, dtype=np.float64)).to(DEV)
    ex = torch.tensor(EXPLORE, dtype=torch.float32, device=DEV)
    parent = torch.full((K,), -7, dtype=torch.int32, device=DEV) if outs[0] else None
    rank = torch.full((K,), -7, dtype=torch.int32, device=DEV) if outs[1] else None
    rc = lib().pcc_pbt_evolve(_p(s), K, n_cut, _p(P), _p(M), _p(V), P.stride(0), n_params, _p(H), _p(ex), seed, generation, _p(parent), _p(rank),
                              _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return P, M, V, H, parent, rank


def _same(got, want, what):
    names = ("params", "adam_m", "adam_v", "hyper", "parent", "rank")
    for name, g, w in zip(names, got, want):
        if g is None:
            continue
        w = torch.from_numpy(np.ascontiguousarray(w)).to(DEV)
        assert g.dtype == w.dtype and torch.equal(_bits(g), _bits(w)), (name, what)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SCORE_KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_evolve_equals_the_reference(shape, kind):
    K, n, stride = shape
    blocks = make_case(K, n, stride, 100 + K)
    rng = np.random.default_rng(K + n)
    for cut in n_cuts(K):
        score = make_scores(kind, K, cut, rng)
        want = evolve_reference(score, cut, *blocks[:3], n, blocks[3], EXPLORE, 9, 4)
        got = _evolve(score, cut, blocks, n, 9, 4)
        _same(got, want, (shape, kind, cut))
        before = [torch.from_numpy(b).to(DEV) for b in blocks]
        keep = torch.from_numpy(want[4] == np.arange(K)).to(DEV)                 # the members the reference does not replace
        for g, b in zip(got[:4], before):
            assert torch.equal(_bits(g[keep]), _bits(b[keep])), (shape, kind, cut)   # bit-identical to before
        for g in got[:3]:
            assert bool((g[:, n:] == PAD).all()), (shape, kind, cut)                # the padding is still the sentinel
        if kind == "all_nan" or cut == 0:
            assert bool(keep.all()) and torch.equal(got[4], torch.arange(K, dtype=torch.int32, device=DEV))
        elif kind != "few_valid" or cut >= 2:
            assert int((~keep).sum()) == cut


@pytest.mark.gpu
def test_same_arguments_same_result_and_other_draws():
    """Two calls on the same inputs agree bit for bit; another generation or seed draws other parents at K = 1024, n_cut = 256 (the
    reference says so for these three draws: tests/test_pbt_cpu.py), and the kernel follows the reference in each."""
    K, n, stride, cut = 1024, 70, 128, 256
    blocks = make_case(K, n, stride, 1)
    score = make_scores("distinct", K, cut, np.random.default_rng(1))
    parents = []
    for seed, gen in DRAWS:
        got = _evolve(score, cut, blocks, n, seed, gen)
        _same(got, evolve_reference(score, cut, *blocks[:3], n, blocks[3], EXPLORE, seed, gen), (seed, gen))
        parents.append(got[4])
    assert not torch.equal(parents[0], parents[1]) and not torch.equal(parents[0], parents[2])
    again = _evolve(score, cut, blocks, n, *DRAWS[0])
    first = _evolve(score, cut, blocks, n, *DRAWS[0])
    for a, b in zip(again, first):
        assert torch.equal(_bits(a), _bits(b))
    big = (5 << 32) | 1                                                          # the seed's high word is the second key word
    _same(_evolve(score, cut, blocks, n, big, 0), evolve_reference(score, cut, *blocks[:3], n, blocks[3], EXPLORE, big, 0), "64-bit seed")


@pytest.mark.gpu
@pytest.mark.parametrize("outs", [(False, False), (True, False), (False, True)], ids=["none", "parent", "rank"])
def test_outputs_may_be_null(outs):
    K, n, stride, cut = 8, 3075, 3136, 2
    blocks = make_case(K, n, stride, 3)
    score = make_scores("distinct", K, cut, np.random.default_rng(3))
    got = _evolve(score, cut, blocks, n, 2, 0, outs=outs)
    assert (got[4] is None) == (not outs[0]) and (got[5] is None) == (not outs[1])
    _same(got, evolve_reference(score, cut, *blocks[:3], n, blocks[3], EXPLORE, 2, 0), outs)


# ------------------------------------------------------------------------------------------------------------ PopulationPPO
POOLS = (2, 8, 32)   # (fixed ring pools: a snapshot needs equal pools)
KP, N_M, T = 4, 128, 8
LRS, ENTS = [1e-3, 3e-4, 1e-4, 3e-5], [0.01, 0.02, 0.0, 0.005]
SCORES = [3, 1, 2, 0]


def _population(seeds=(0, 1, 2, 3)):
    env = pcc_rl_amd.BatchedNetworkEnv(KP * N_M, device=DEV, seed=21, ring_pools=POOLS)
    return env, PopulationPPO(env, KP, horizon=T, lr=LRS, ent_coef=ENTS, seeds=list(seeds))


def _fixed_iteration(pop, seed):
    """collect() + update() with the noise and the permutations of `seed`"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    N = KP * N_M
    noise = torch.randn((T, N), device=DEV, generator=g)
    perms = [population_permutations(T, N, KP, device=DEV, generator=g) for _ in range(pop.epochs)]
    batch = pop.collect(noise=noise)
    pop.update(*batch[:5], perms=perms)


def _reference_hyper(pop, scores, cut, seed, generation, **kw):
    K, z = pop.members, np.zeros((pop.members, 64), dtype=np.float32)
    return evolve_reference(np.asarray(scores, dtype=np.float64), cut, z, z, z, 1, pop.hyper.cpu().numpy(), explore_matrix(**kw), seed, generation)


@pytest.mark.gpu
def test_population_evolve():
    """evolve([3, 1, 2, 0], frac=0.25) after one iteration: member 3 becomes member 0 -- policy module, moments, the perturbed
    hyper row of the reference -- and members 0 .. 2 stay as they were."""
    env, pop = _population()
    _fixed_iteration(pop, 1)
    flat, m, v, hyper = pop.flat.clone(), pop.adam_m.clone(), pop.adam_v.clone(), pop.hyper.clone()
    assert bool((m[0] != 0).any()) and not torch.equal(flat[3], flat[0])
    want = _reference_hyper(pop, SCORES, 1, 0, 0)
    with pytest.raises(ValueError, match="frac"):
        pop.evolve(SCORES, frac=0.6)
    with pytest.raises(ValueError, match="frac"):
        pop.evolve(SCORES, frac=-0.1)
    assert pop.generation == 0 and pop.hyper_rows is not None
    parent, rank = pop.evolve(SCORES, frac=0.25)
    torch.cuda.synchronize()
    assert parent.dtype == torch.int32 and parent.tolist() == [0, 1, 2, 0] and rank.tolist() == [0, 2, 1, 3]
    assert want[4].tolist() == [0, 1, 2, 0]
    n = pop.n_params
    for new, was in ((pop.flat, flat), (pop.adam_m, m), (pop.adam_v, v)):
        assert torch.equal(_bits(new[3, :n]), _bits(was[0, :n]))
        assert torch.equal(_bits(new[:3]), _bits(was[:3])) and torch.equal(_bits(new[:, n:]), _bits(was[:, n:]))
    for a, b in zip(pop.policies[3].parameters(), pop.policies[0].parameters()):   # (the modules are views of the rows)
        assert torch.equal(a, b)
    assert torch.equal(_bits(pop.hyper), _bits(torch.from_numpy(want[3]).to(DEV)))
    assert torch.equal(pop.hyper[:3], hyper[:3]) and torch.equal(pop.hyper[3, [1, 3, 4, 5, 6, 7]], hyper[0, [1, 3, 4, 5, 6, 7]])
    assert float(pop.hyper[3, 0]) in (float(np.float32(LRS[0]) * np.float32(0.8)), float(np.float32(LRS[0]) * np.float32(1.2)))
    assert pop.generation == 1 and pop.hyper_rows is None
    assert pop.hypers() == pop.hyper.tolist() and len(pop.hypers()) == KP and len(pop.hypers()[0]) == 8
    # a tensor of scores, other columns, bounds, another seed: the reference's hyper block and parents again
    s = torch.tensor([0.5, float("nan"), 2.0, 1.0], device=DEV)
    kw = dict(factors=(0.5, 2.0), explore=("lr", "gamma"), bounds={"lr": (2e-4, 4e-4), "gamma": (0.9, 0.999)})
    want = _reference_hyper(pop, s.tolist(), 2, 77, 1, **kw)
    parent, _ = pop.evolve(s, frac=0.5, seed=77, **kw)
    assert parent.tolist() == want[4].tolist() and parent.tolist()[1] in (2, 3) and parent.tolist()[0] in (2, 3)
    assert torch.equal(_bits(pop.hyper), _bits(torch.from_numpy(want[3]).to(DEV)))
    assert pop.generation == 2
    env.close()


@pytest.mark.gpu
def test_training_after_evolve_equals_rows_copied_by_hand():
    """The iteration after an evolve -- fixed noise and permutations -- ends with the bits of a second population whose rows were
    copied with plain torch indexing and whose hyper block is the reference's."""
    env_a, a = _population()
    env_b, b = _population()
    _fixed_iteration(a, 1)
    _fixed_iteration(b, 1)
    assert torch.equal(a.flat, b.flat)
    want = _reference_hyper(b, SCORES, 1, 5, 0)
    parent, _ = a.evolve(SCORES, frac=0.25, seed=5)
    assert parent.tolist() == want[4].tolist() == [0, 1, 2, 0]
    with torch.no_grad():
        for block in (b.flat, b.adam_m, b.adam_v):
            block[3, :b.n_params] = block[0, :b.n_params]
        b.hyper.copy_(torch.from_numpy(want[3]).to(DEV))
    _fixed_iteration(a, 2)
    _fixed_iteration(b, 2)
    torch.cuda.synchronize()
    env_a.check_flags()
    env_b.check_flags()
    for name in ("flat", "adam_m", "adam_v", "hyper"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    assert torch.isfinite(a.flat[:, :a.n_params]).all() and not torch.equal(a.flat[3], a.flat[0])   # (other envs: the twins part again)
    env_a.close(); env_b.close()


@pytest.mark.gpu
def test_resume_after_evolve_is_bit_for_bit():
    env_a, a = _population()
    a.iterate()
    a.evolve(SCORES, frac=0.25, seed=3)
    sd = a.state_dict()
    assert sd["generation"] == 1 and sd["format"] == "population-1"
    parents, returns = [], []

    def go_on(pop):   # (one after the other: the rollout's noise and the permutations come from torch's global device generator)
        returns.append(pop.iterate()["mean_step_reward"])
        parents.append(pop.evolve([1, 3, 0, 2], frac=0.5, seed=3)[0])

    go_on(a)
    env_b, b = _population(seeds=(9, 9, 9, 9))                                  # (another start: everything comes from the state)
    b.load_state_dict(sd)
    assert b.generation == 1
    go_on(b)
    torch.cuda.synchronize()
    assert returns[0] == returns[1] and torch.equal(parents[0], parents[1]) and a.generation == b.generation == 2
    assert int((parents[0] != torch.arange(KP, dtype=torch.int32, device=DEV)).sum()) == 2
    for name in ("flat", "adam_m", "adam_v", "hyper", "obs"):
        assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), name
    old = {k: v for k, v in sd.items() if k != "generation"}                     # a checkpoint from before evolve() existed
    b.load_state_dict(old)
    assert b.generation == 0
    env_a.close(); env_b.close()
