"""Gradient-norm clipping and the non-finite guard on the GPU (include/pcc_policy.h: pcc_ppo_minibatch_step_clip_pop; DESIGN.md section
24; pcc_rl_amd.gradclip, PPO / PopulationPPO(max_grad_norm=...)).  The reference of everything that does not clip is
pcc_ppo_minibatch_step_pop itself, bit for bit; the norm and the coefficient are held to the numpy model of
tests/models/grad_clip_model.py (the sum of squares bit for bit: its order is the contract), the clipped Adam step to the model's
float64 restatement within its derived bounds.

Shapes: (30, 32, 16) the fixed MFMA kernel, 3075 = 12 * 256 + 3 parameters (a 3-lane tail); (5, 7, 3) tiled, 141 parameters (lanes
without a parameter); (128, 64, 64) tiled, 24 963, the largest of the domain.  96 envs x 8 rows, K in {1, 3} members (256 samples per
member at K = 3), minibatch start 17, count 200, param_stride the next multiple of 64.  A case's inputs and the unclipped reference are
computed once and never written."""
import ctypes
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import grad_clip_model as model  # noqa: E402

import pcc_rl_amd  # noqa: E402
from pcc_rl_amd.native import lib  # noqa: E402
from pcc_rl_amd.ppo import PPO, MlpPolicy, PopulationPPO, population_permutations  # noqa: E402

DEV = "cuda:0"
SHAPES = [(30, 32, 16), (5, 7, 3), (128, 64, 64)]
MEMBERS = [1, 3]
N_ENVS, T, START, COUNT = 96, 8, 17, 200
PAD = 7.0      # what the padding of every block and of the clip rows holds before a call -- and after it
BIG = 1e30     # a limit nobody reaches
LRS = [1e-3, 3e-4, 2e-3]
CLIP_STRIDE = 9
_ids = lambda s: "%d-%d-%d" % s if isinstance(s, tuple) else "K%d" % s
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
_bits = lambda x: x.contiguous().view(torch.int32)
f32 = lambda x: float(np.float32(x))
BLOCKS = ("params", "m", "v", "grad", "stats")

both = lambda f: pytest.mark.gpu(pytest.mark.parametrize("K", MEMBERS, ids=_ids)(pytest.mark.parametrize("shape", SHAPES, ids=_ids)(f)))
shapes = lambda f: pytest.mark.gpu(pytest.mark.parametrize("shape", SHAPES, ids=_ids)(f))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


# ---------------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def _case(shape, K):
    """One rollout's flattened rows, K policies and their permutations.  Never written: every run works on clones."""
    D, h1, h2 = shape
    n_par = 2 * (h1 * D + h1 + h2 * h1 + 2 * h2 + 1) + 1
    stride = (n_par + 63) // 64 * 64
    block = torch.full((K, stride), PAD, device=DEV)
    g = torch.Generator().manual_seed(1000 * D + K)
    n = T * N_ENVS
    obs = torch.randn(n, D, generator=g).to(DEV)
    act = (0.5 * torch.randn(n, generator=g)).to(DEV)
    adv = torch.randn(n, generator=g).to(DEV)
    ret = (2.0 * torch.randn(n, generator=g)).to(DEV)
    logp = torch.zeros(n, device=DEV)
    perm = population_permutations(T, N_ENVS, K, generator=g).to(DEV)
    with torch.no_grad():   # log-probabilities near each member's own policy: ratios around 1
        for m in range(K):
            torch.manual_seed(50 + m)
            pol = MlpPolicy(D, 1, (h1, h2))
            pol.log_std.fill_(-0.3 - 0.2 * m)
            block[m, :n_par] = pol.flat_params().to(DEV)
            idx = perm[m]
            logp[idx] = pol.to(DEV).dist(obs[idx]).log_prob(act[idx].unsqueeze(1)).sum(-1) + 0.15 * torch.randn(idx.numel(), generator=g).to(DEV)
    sf = lib().pcc_ppo_scratch_floats(D, h1, h2)
    torch.cuda.synchronize()
    return types.SimpleNamespace(shape=shape, K=K, n_par=n_par, stride=stride, block=block, obs=obs, act=act, adv=adv, ret=ret, logp=logp,
                                 perm=perm, scratch_floats=sf)


def _state(c):
    """Fresh blocks: the case's parameters, zero moments, poisoned gradient and statistics; the clip rows with zeroed accumulators."""
    full = lambda: torch.full((c.K, c.stride), PAD, device=DEV)
    st = {"params": c.block.clone(), "m": full(), "v": full(), "grad": full(), "stats": torch.full((c.K, 4), float("nan"), device=DEV)}
    st["m"][:, :c.n_par] = 0.0
    st["v"][:, :c.n_par] = 0.0
    st["clip"] = torch.full((c.K, CLIP_STRIDE), PAD, dtype=torch.float64, device=DEV)
    st["clip"][:, :4] = float("nan")
    st["clip"][:, 4:8] = 0.0
    st["hyper_grad"] = torch.full((c.K, 8), float("nan"), device=DEV)
    st["scratch"] = torch.empty(c.K * c.scratch_floats, device=DEV)
    return st


def _hyper(c, limits=0.0, lrs=None):
    limits = [limits] * c.K if not isinstance(limits, (list, tuple)) else limits
    lrs = LRS[:c.K] if lrs is None else lrs
    return torch.tensor([[lrs[m], 0.2, 0.01, 0.99, 0.95, limits[m], 0.0, 0.0] for m in range(c.K)], dtype=torch.float32, device=DEV)


def _plain(c, st, hyper, t):
    D, h1, h2 = c.shape
    rc = lib().pcc_ppo_minibatch_step_pop(_p(c.obs), _p(c.act), _p(c.logp), _p(c.adv), _p(c.ret), _p(c.perm), c.perm.stride(0), START, COUNT,
                                          D, h1, h2, _p(st["params"]), _p(st["m"]), _p(st["v"]), c.stride, c.K, _p(hyper), t, 0.9, 0.999, 1e-5,
                                          _p(st["scratch"]), _p(st["grad"]), _p(st["stats"]), _stream())
    assert rc == 0
    torch.cuda.synchronize()


def _clipped(c, st, hyper, t, adv=None, ret=None, member=None):
    """One call of the new entry on the whole population, or (member=m) on member m alone as a population of one: its rows of every
    block, its permutation, its row of hyper."""
    D, h1, h2 = c.shape
    row = (lambda x: x) if member is None else (lambda x: x[member])
    rc = lib().pcc_ppo_minibatch_step_clip_pop(
        _p(c.obs), _p(c.act), _p(c.logp), _p(c.adv if adv is None else adv), _p(c.ret if ret is None else ret), _p(row(c.perm)),
        c.perm.stride(0), START, COUNT, D, h1, h2, _p(row(st["params"])), _p(row(st["m"])), _p(row(st["v"])), c.stride,
        c.K if member is None else 1, _p(row(hyper)), t, 0.9, 0.999, 1e-5, _p(st["scratch"]), _p(row(st["grad"])), _p(row(st["stats"])),
        _p(row(st["hyper_grad"])), _p(row(st["clip"])), CLIP_STRIDE, _stream())
    assert rc == 0
    torch.cuda.synchronize()


def _snap(st, names=BLOCKS + ("clip",)):
    return {n: st[n].clone() for n in names}


def _same(a, b, names=BLOCKS, member=None):
    for n in names:
        x, y = (a[n], b[n]) if member is None else (a[n][member], b[n][member])
        if not torch.equal(_bits(x), _bits(y)):
            return False
    return True


def _padding_kept(c, st):
    return all(bool((st[n][:, c.n_par:] == PAD).all()) for n in ("params", "m", "v", "grad")) and bool((st["clip"][:, 8:] == PAD).all())


@functools.lru_cache(maxsize=None)
def _reference(shape, K):
    """Three consecutive steps of the unclipped entry from the fresh state: the snapshots after each."""
    c = _case(shape, K)
    st, hyper, out = _state(c), _hyper(c), []
    for t in (1, 2, 3):
        _plain(c, st, hyper, t)
        out.append(_snap(st, BLOCKS))
    return out


def _norms(c, grad):
    """The model's (sumsq, norm) of every member's row of a gradient block."""
    g = grad.cpu().numpy()
    sums = [model.ordered_sumsq(g[m, :c.n_par]) for m in range(c.K)]
    return sums, [float(np.sqrt(s)) for s in sums]


def _half_the_smallest_norm(shape, K):
    c = _case(shape, K)
    return f32(0.5 * min(_norms(c, _reference(shape, K)[0]["grad"])[1]))


@functools.lru_cache(maxsize=None)
def _clipped_run(shape, K):
    """Two consecutive steps with every member's limit at half the smallest member norm of the first gradient: per step the state
    before, the state after."""
    c = _case(shape, K)
    limit = _half_the_smallest_norm(shape, K)
    st, hyper, out = _state(c), _hyper(c, limit), []
    for t in (1, 2):
        before = _snap(st)
        _clipped(c, st, hyper, t)
        out.append((before, _snap(st)))
    assert _padding_kept(c, st)
    return limit, out


def _neighbour64(a, b):
    return a == b or abs(a - b) <= np.spacing(np.float64(b))


def _neighbour32(a, b):
    return np.float32(a) == np.float32(b) or abs(float(np.float32(a)) - float(np.float32(b))) <= float(np.spacing(np.float32(b)))


# ------------------------------------------------------------------------------------------------------------ 1. unclipped
@both
@pytest.mark.parametrize("limit", [0.0, BIG], ids=["guard-only", "limit-1e30"])
def test_an_unclipped_step_keeps_the_bits(shape, K, limit):
    c, ref = _case(shape, K), _reference(shape, K)
    st, hyper = _state(c), _hyper(c, limit)
    for t in (1, 2, 3):
        _clipped(c, st, hyper, t)
        assert _same(st, ref[t - 1]), (shape, K, limit, t, [n for n in BLOCKS if not _same(st, ref[t - 1], (n,))])
        rows = st["clip"].tolist()
        sums, _ = _norms(c, st["grad"])
        for m in range(c.K):
            # state 0, c == 1, t steps, none clipped or skipped (max_norm_seen: test_accumulators_and_determinism)
            assert rows[m][0] == sums[m] and rows[m][2:7] == [1.0, 0.0, float(t), 0.0, 0.0] and rows[m][7] >= rows[m][1] > 0.0, (m, rows[m])
    assert _padding_kept(c, st)
    assert torch.equal(st["hyper_grad"][:, 1:], hyper[:, 1:]) and bool((st["hyper_grad"][:, 0] == 0.0).all())
    assert torch.isfinite(ref[2]["params"][:, :c.n_par]).all() and not torch.equal(ref[2]["params"], c.block)


# ------------------------------------------------------------------------------------------------- 2. norm and coefficient
@both
def test_norm_and_coefficient(shape, K):
    c, ref = _case(shape, K), _reference(shape, K)
    limit, run = _clipped_run(shape, K)
    _, after = run[0]
    assert _same(after, ref[0], ("grad", "stats"))          # the gradient launch is the unclipped entry's
    sums, norms = _norms(c, after["grad"])
    assert limit > 0.0 and all(limit < 0.51 * x for x in norms)
    for m, row in enumerate(after["clip"].tolist()):
        state, coef, norm = model.decide(sums[m], LRS[m], limit)
        assert state == model.CLIPPED
        assert row[0] == sums[m], (m, row[0], sums[m])       # bit-equal: the order of the sum is the contract
        assert _neighbour64(row[1], norm), (m, row[1], norm)
        assert _neighbour32(row[2], coef) and row[2] == float(np.float32(row[2])), (m, row[2], float(coef))
        assert row[3:8] == [1.0, 1.0, 1.0, 0.0, row[1]], (m, row)


# ------------------------------------------------------------------------------------------------------- 3. clipped Adam
@both
def test_clipped_adam_within_its_bounds(shape, K):
    c = _case(shape, K)
    limit, run = _clipped_run(shape, K)
    n = c.n_par
    worst = [0.0, 0.0, 0.0]
    for t, (before, after) in enumerate(run, 1):
        G, rows = after["grad"].cpu(), after["clip"].tolist()
        for m in range(c.K):
            coef = torch.tensor(rows[m][2], dtype=torch.float32)
            gc = (G[m, :n] * coef).numpy()
            assert gc.dtype == np.float32
            if t == 1:
                assert rows[m][3] == 1.0 and 0.0 < rows[m][2] < 0.51
            if rows[m][3] == 1.0:   # |gc| <= c norm (1 + u), c <= M / norm (1 + u) (1 + 2^-53): inside M (1 + 4u)
                assert float(np.sqrt((gc.astype(np.float64) ** 2).sum())) <= limit * (1.0 + 4.0 * model.U), (t, m)
            cut = lambda s: [s[k][m, :n].cpu().numpy() for k in ("m", "v", "params")]
            errs = model.adam_errors(t, gc, cut(before), cut(after), f32(LRS[m]))
            print("%s K%d t%d member %d: adam m, v, step error / bound = %.3f %.3f %.3f" % ((shape, K, t, m) + errs))
            assert max(errs) <= 1.0, (shape, K, t, m, errs)
            worst = [max(a, b) for a, b in zip(worst, errs)]
            assert not np.array_equal(cut(before)[2], cut(after)[2])
    assert worst[2] > 0.0


# ------------------------------------------------------------------------------------------------------ 4. mixed members
@shapes
def test_mixed_members_and_each_member_alone(shape):
    K = 3
    c, ref = _case(shape, K), _reference(shape, K)
    small = f32(0.5 * _norms(c, ref[0]["grad"])[1][1])
    hyper = _hyper(c, [0.0, small, BIG])
    st = _state(c)
    mixed = []
    for t in (1, 2):
        _clipped(c, st, hyper, t)
        mixed.append(_snap(st))
        for m in (0, 2):
            assert _same(st, ref[t - 1], member=m), (t, m)
            assert st["clip"][m, 3].item() == 0.0
    # member 1: clipped at the first step (its limit is half that step's norm), two steps applied, none skipped
    assert mixed[0]["clip"][1, 3].item() == 1.0 and st["clip"][1, 4].item() == 2.0 and st["clip"][1, 5].item() >= 1.0 and st["clip"][1, 6].item() == 0.0
    assert _same(mixed[0], ref[0], ("grad", "stats"), member=1) and not _same(mixed[0], ref[0], ("params",), member=1)
    assert not _same(mixed[0], ref[0], ("m",), member=1) and not _same(mixed[0], ref[0], ("v",), member=1)
    assert _padding_kept(c, st)
    fresh = _state(c)
    for m in range(K):   # the same calls on member m alone: a population of one on its rows
        alone = _state(c)
        alone["scratch"] = torch.empty(c.scratch_floats, device=DEV)
        for t in (1, 2):
            _clipped(c, alone, hyper, t, member=m)
            assert _same(alone, mixed[t - 1], BLOCKS + ("clip",), member=m), (m, t)
        for other in range(K):   # ... which touches nobody else's
            if other != m:
                assert _same(alone, fresh, ("params", "m", "v", "grad", "clip"), member=other), (m, other)


# ---------------------------------------------------------------------------------------------- 5. a non-finite gradient
@shapes
def test_a_non_finite_gradient_is_skipped(shape):
    """One of member 1's selected samples gets a NaN advantage and a NaN return.  (The advantage alone does not reach the gradient:
    the gradient kernels pass a sample's policy term on only where surr1 <= surr2 holds, which a NaN fails, so that sample's policy
    term is 0 and the NaN shows in the pg statistic alone; the return enters the value error directly.)  Plain arithmetic on a
    NaN input."""
    K = 3
    c = _case(shape, K)
    limit, run = _clipped_run(shape, K)
    adv, ret = c.adv.clone(), c.ret.clone()
    bad = c.perm[1, START + 5]
    adv[bad], ret[bad] = float("nan"), float("nan")
    st, hyper = _state(c), _hyper(c, limit)
    start = _snap(st)
    _clipped(c, st, hyper, 1, adv=adv, ret=ret)
    row = st["clip"][1].tolist()
    assert not torch.isfinite(st["grad"][1, :c.n_par]).all()
    assert np.isnan(row[0]) and np.isnan(row[1]) and row[2:8] == [1.0, 2.0, 0.0, 0.0, 1.0, 0.0], row   # skipped; the NaN norm is not "seen"
    assert _same(st, start, ("params", "m", "v"), member=1)
    for m in (0, 2):
        assert _same(st, run[0][1], BLOCKS + ("clip",), member=m), m
    assert _padding_kept(c, st)
    _clipped(c, st, hyper, 2)   # the next step, on finite rows again, is taken
    assert st["clip"][1, 3:7].tolist() == [1.0, 1.0, 1.0, 1.0] and not _same(st, start, ("params",), member=1)
    assert torch.isfinite(st["params"][:, :c.n_par]).all() and torch.isfinite(st["m"][:, :c.n_par]).all()


# ------------------------------------------------------------------------------------------------- 6. a stopped member
@both
def test_a_stopped_member_is_gradient_only(shape, K):
    c, ref = _case(shape, K), _reference(shape, K)
    who = K // 2
    lrs = list(LRS[:K])
    lrs[who] = 0.0
    st, hyper = _state(c), _hyper(c, _half_the_smallest_norm(shape, K), lrs)
    start = _snap(st)
    _clipped(c, st, hyper, 1)
    row = st["clip"][who].tolist()
    sums, norms = _norms(c, st["grad"])
    assert _same(st, start, ("params", "m", "v"), member=who)
    assert _same(st, ref[0], ("grad", "stats"))
    assert row[0] == sums[who] and _neighbour64(row[1], norms[who]) and row[1] > 0.0        # the norm is still reported
    assert row[2:8] == [1.0, 3.0, 0.0, 0.0, 0.0, row[1]], row
    for m in range(K):
        if m != who:
            assert _same(st, _clipped_run(shape, K)[1][0][1], BLOCKS + ("clip",), member=m), m
    assert _padding_kept(c, st)


# ------------------------------------------------------------------------------------- 7. accumulators and determinism
@both
def test_accumulators_and_determinism(shape, K):
    c, ref = _case(shape, K), _reference(shape, K)
    _, first = _norms(c, ref[0]["grad"])
    limits = [f32(0.97 * first[0])] if K == 1 else [f32(0.5 * first[0]), BIG, f32(0.97 * first[2])]
    hyper = _hyper(c, limits)
    runs = []
    for _ in range(2):
        st = _state(c)
        want = [[0.0] * 8 for _ in range(K)]
        seen = [[] for _ in range(K)]
        for t in range(1, 6):
            _clipped(c, st, hyper, t)
            sums, _ = _norms(c, st["grad"])
            rows = st["clip"].tolist()
            for m in range(K):
                state = model.accumulate(want[m], sums[m], LRS[m], limits[m])
                seen[m].append(rows[m][1])
                assert rows[m][0] == sums[m] and rows[m][3] == float(state), (t, m, rows[m], want[m])
                assert rows[m][4:7] == want[m][4:7], (t, m, rows[m], want[m])
                assert rows[m][7] == max(seen[m]) and _neighbour64(rows[m][7], want[m][7]), (t, m, rows[m], want[m])
        assert _padding_kept(c, st)
        runs.append(_snap(st))
    assert _same(runs[0], runs[1], BLOCKS) and torch.equal(runs[0]["clip"], runs[1]["clip"])
    rows = runs[0]["clip"].tolist()
    assert all(r[4] == 5.0 and r[6] == 0.0 for r in rows)
    if K == 3:
        assert rows[0][5] == 5.0 and rows[1][5] == 0.0
    print("%s K%d: clipped steps %s of 5" % (shape, K, [r[5] for r in rows]))


# ------------------------------------------------------------------------------------------------------------ 8. trainers
POOLS = (2, 8, 32)   # (fixed ring pools: the library's default depends on the free device memory, and a snapshot needs equal pools)
TR_ENVS, HORIZON = 64, 8
NAMES = ("flat", "adam_m", "adam_v")
NEW_KEYS = ["clipped_steps", "grad_norm", "max_grad_norm_seen", "skipped_steps"]


def _env(seed):
    return pcc_rl_amd.BatchedNetworkEnv(TR_ENVS, device=DEV, seed=seed, ring_pools=POOLS)


def _train(make, iters=2):
    env, agent = make()
    stats = [agent.iterate() for _ in range(iters)]
    torch.cuda.synchronize()
    out = {n: getattr(agent, n).clone() for n in NAMES}
    out.update(adam_t=agent.adam_t, stats=stats, hyper=agent.hyper.clone() if getattr(agent, "hyper", None) is not None else None)
    env.close()
    return out


def _ppo(**kw):
    def make():
        env = _env(42)
        return env, PPO(env, horizon=HORIZON, seed=2, **kw)
    return make


def _pop(**kw):
    def make():
        env = _env(44)
        return env, PopulationPPO(env, 4, horizon=HORIZON, seeds=[5, 6, 7, 8], lr=[1e-3, 3e-3, 1e-3, 3e-4], **kw)
    return make


@functools.lru_cache(maxsize=None)
def _plain_ppo():
    return _train(_ppo())


@pytest.mark.gpu
def test_ppo_with_a_limit_nobody_reaches_is_ppo():
    plain = _plain_ppo()
    for kw in ({"max_grad_norm": BIG}, {"max_grad_norm": 0.0}, {"max_grad_norm": BIG, "target_kl": 1e9}):
        got = _train(_ppo(**kw))
        assert _same(got, plain, NAMES) and got["adam_t"] == plain["adam_t"], kw
        for a, b in zip(got["stats"], plain["stats"]):
            assert all(a[k] == b[k] for k in b), kw
            assert sorted(k for k in set(a) - set(b) if k in NEW_KEYS) == NEW_KEYS
            assert a["clipped_steps"] == 0 and a["skipped_steps"] == 0 and 0.0 < a["grad_norm"] <= a["max_grad_norm_seen"], a
        assert got["hyper"][0, 5].item() == f32(kw["max_grad_norm"])


@pytest.mark.gpu
def test_population_with_a_limit_nobody_reaches_is_the_population():
    plain = _train(_pop())
    assert plain["hyper"][:, 5].tolist() == [0.0] * 4            # None: column 5 stays 0
    got = _train(_pop(max_grad_norm=[BIG, 0.0, BIG, BIG]))
    assert _same(got, plain, NAMES) and got["adam_t"] == plain["adam_t"]
    assert got["hyper"][:, 5].tolist() == [f32(BIG), 0.0, f32(BIG), f32(BIG)]
    s = got["stats"][-1]
    assert s["clipped_steps"] == [0] * 4 and s["skipped_steps"] == [0] * 4 and all(0.0 < a <= b for a, b in zip(s["grad_norm"], s["max_grad_norm_seen"]))
    assert all(s[k] == plain["stats"][-1][k] for k in plain["stats"][-1])


@pytest.mark.gpu
def test_ppo_under_a_limit_clips():
    plain = _plain_ppo()
    seen = _train(_ppo(max_grad_norm=BIG), iters=1)["stats"][0]["max_grad_norm_seen"]
    limit = 0.5 * seen                                            # below the first update's largest norm: that step, or an earlier one, clips
    got = _train(_ppo(max_grad_norm=limit))
    assert got["stats"][0]["clipped_steps"] > 0 and got["stats"][0]["skipped_steps"] == 0, got["stats"][0]
    assert not _same(got, plain, ("flat",)) and got["adam_t"] == plain["adam_t"]
    assert torch.isfinite(got["flat"]).all()
    guarded = _train(_ppo(max_grad_norm=limit, target_kl=1e9))    # the hyper_live path, a target nobody reaches: the same steps
    assert guarded["stats"][0]["clipped_steps"] == got["stats"][0]["clipped_steps"] and guarded["stats"][0]["epochs_run"] == 4
    assert _same(guarded, got, NAMES)
    stopped = _train(_ppo(max_grad_norm=limit, target_kl=1e-12))  # stopped after the first epoch: the later steps are gradient-only
    assert stopped["stats"][0]["epochs_run"] == 1 and not _same(stopped, got, ("flat",))
    one = _train(_ppo(max_grad_norm=limit, epochs=1), iters=1)
    assert _same(_train(_ppo(max_grad_norm=limit, target_kl=1e-12), iters=1), one, NAMES)


@pytest.mark.gpu
def test_ppo_follows_a_limit_changed_after_construction():
    """The limit is read at every update, as lr, clip and ent_coef are: a schedule that sets agent.max_grad_norm is obeyed."""
    env, agent = _ppo(max_grad_norm=BIG)()
    assert agent.max_grad_norm == BIG
    assert agent.iterate()["clipped_steps"] == 0
    agent.max_grad_norm = 1e-6
    stats = agent.iterate()
    assert stats["clipped_steps"] == 4 and agent.hyper[0, 5].item() == f32(1e-6)      # 4 epochs of one minibatch each
    agent.max_grad_norm = -1.0
    with pytest.raises(ValueError, match="max_grad_norm"):
        agent.iterate()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ppo", "population"])
def test_resume_is_bit_for_bit_with_the_option_on(kind):
    make = _ppo(max_grad_norm=0.05) if kind == "ppo" else _pop(max_grad_norm=[0.05, 0.5, 0.0, BIG])
    env, a = make()
    a.iterate()
    sd = a.state_dict()
    want_stats = a.iterate()
    torch.cuda.synchronize()
    want = {n: getattr(a, n).clone() for n in NAMES + ("obs",)}
    env.close()
    plain = (_ppo() if kind == "ppo" else _pop())()
    assert sorted(set(sd) - set(plain[1].state_dict())) == []    # no new checkpoint state
    plain[0].close()
    env, b = make()
    b.iterate()
    b.iterate()                                                   # (another state: everything comes from the checkpoint)
    b.load_state_dict(sd)
    got_stats = b.iterate()
    torch.cuda.synchronize()
    for n in NAMES + ("obs",):
        assert torch.equal(_bits(getattr(b, n)), _bits(want[n])), n
    assert repr(got_stats) == repr(want_stats)
    clipped = want_stats["clipped_steps"]
    assert (clipped > 0) if kind == "ppo" else (clipped[0] > 0 and clipped[2] == 0 and clipped[3] == 0), want_stats
    env.close()


@pytest.mark.gpu
def test_a_replaced_member_takes_its_parents_limit():
    limits = [0.25, 0.5, 1.0, 2.0]
    env, pop = _pop(max_grad_norm=limits)()
    pop.iterate()
    parent, _ = pop.evolve(scores=[3.0, 1.0, 4.0, 2.0], frac=0.25, seed=1)
    parent = parent.tolist()
    assert parent == [0, 2, 2, 3]                                 # the worst member takes over the best
    assert pop.hyper[:, 5].tolist() == [limits[p] for p in parent]
    stats = pop.iterate()                                         # ... and trains under it
    assert len(stats["grad_norm"]) == 4 and all(np.isfinite(stats["grad_norm"]))
    parent, _ = pop.evolve(scores=[3.0, 1.0, 4.0, 2.0], frac=0.25, seed=1, explore=("max_grad_norm",), factors=(0.5, 0.5),
                           bounds={"max_grad_norm": (0.75, 10.0)})
    assert pop.hyper[:, 5].tolist() == [0.25, 0.75, 1.0, 2.0]     # 1.0 * 0.5, held at the lower bound
    env.close()
