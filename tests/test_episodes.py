"""The episode ledger on the GPU (include/pcc_policy.h: pcc_episode_update_pop and its stand-alone form; pcc_rl_amd.episodes.
EpisodeLedger; PPO / PopulationPPO with track_episodes=True; pcc_rl_amd.evaluate).

The reference is the numpy restatement of tests/models/episode_ledger_model.py.  carry, carry_len, last and last_len are compared
bit for bit; episodes, steps, min and max by value, exactly; sum and sumsq against the exactly rounded sum of the model's episode
list within E 2^-52 sum|v| (sum v^2 for sumsq), E the member's episodes since its row was zero: the first-order bound
(E - 1) 2^-53 sum|v| of any summation order, doubled for the merge with the existing row (model.sum_bounds).  The largest
observed ratio of error to bound is printed by every check (0.33 over this file, at one env per member where E is 2 .. 9: DESIGN.md
section 21).
Synthetic inputs: rewards 3 randn, done Bernoulli(p), step records randn times a scale per column.  Shapes (T, N, members, C):
one env; less than a wavefront; across a workgroup; a member size that is no multiple of the wavefront with all 8 channels; one
env per member at the member limit; the reference's episode length with done at the last step only."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import pcc_rl_amd
from pcc_rl_amd import evaluate as evaluate_module
from pcc_rl_amd.episodes import EpisodeLedger
from pcc_rl_amd.evaluate import evaluate
from pcc_rl_amd.native import lib
from pcc_rl_amd.ppo import PPO, PopulationPPO

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import episode_ledger_model as model  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 1, 1, 1), (5, 63, 1, 1), (7, 257, 1, 3), (9, 6 * 65, 6, 8), (4, 1024, 1024, 2)]
IDS = lambda s: "%d-%d-%d-%d" % s
COLS = [6, 0, 17, 2, 5, 1, 18]          # the step-record columns of channels 1 .. 7: reward, sent, latency ratio, ...
SCALE = (1.0, 1e3, 1e-3, 50.0)          # per column, cyclically
PAD, POISON = 3, -7777.25               # doubles behind every totals row, and what they hold
POOLS = (2, 8, 32)                      # (fixed ring pools: a snapshot needs equal pools)
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _inputs(T, N, p, seed):
    rng = np.random.default_rng(seed)
    reward = (3.0 * rng.standard_normal((T, N))).astype(np.float32)
    done = (rng.random((T, N)) < p).astype(np.uint8)
    steps = rng.standard_normal((T, N, model.STEP_COLS)) * np.resize(np.array(SCALE), model.STEP_COLS)
    return reward, done, steps


class _State(object):
    """The caller-owned buffers of one ledger on the device, the totals rows with PAD poisoned doubles behind them."""

    def __init__(self, N, K, C, last=True, last_len=True):
        self.N, self.K, self.C = N, K, C
        self.cols = (ctypes.c_int32 * 7)(*COLS)
        self.carry = torch.zeros((N, C), dtype=torch.float64, device=DEV)
        self.carry_len = torch.zeros(N, dtype=torch.int32, device=DEV)
        self.last = torch.zeros((N, C), dtype=torch.float64, device=DEV) if last else None
        self.last_len = torch.zeros(N, dtype=torch.int32, device=DEV) if last_len else None
        self.totals = torch.zeros((K, 2 + 4 * C + PAD), dtype=torch.float64, device=DEV)
        self.totals[:, 2 + 4 * C:] = POISON
        need = lib().pcc_episode_scratch_doubles(N, K, C)
        assert need > 0
        self.scratch = torch.full((need,), float("nan"), dtype=torch.float64, device=DEV)

    def update(self, reward, done, steps, alone=False):
        """The library call on device copies of numpy rows (steps: None with C == 1 passes NULL)."""
        r, d = torch.from_numpy(reward).to(DEV), torch.from_numpy(done).to(DEV)
        s = None if steps is None else torch.from_numpy(steps).to(DEV)
        T = reward.shape[0]
        head = (_p(r), _p(d), _p(s), self.cols if s is not None else None, self.C, T, self.N)
        tail = (_p(self.carry), _p(self.carry_len), _p(self.last), _p(self.last_len), _p(self.totals), self.totals.stride(0),
                _p(self.scratch), _stream())
        if alone:
            assert self.K == 1
            rc = lib().pcc_episode_update(*(head + tail))
        else:
            rc = lib().pcc_episode_update_pop(*(head + (self.K,) + tail))
        assert rc == 0
        torch.cuda.synchronize()

    def tensors(self):
        return [t for t in (self.carry, self.carry_len, self.last, self.last_len, self.totals) if t is not None]


def _model(N, K, C):
    led = model.Ledger(N, K, COLS[:C - 1], totals_stride=2 + 4 * C + PAD)
    led.totals[:, 2 + 4 * C:] = POISON
    return led


def _check(st, led, what, prior=None):
    """The device's buffers against the model's: bits, exact values, and sum / sumsq within the bound; returns the largest ratio
    of error to bound."""
    C = st.C
    dev = lambda a: torch.from_numpy(a).to(DEV)
    assert torch.equal(st.carry, dev(led.carry)) and torch.equal(st.carry_len, dev(led.carry_len)), what
    if st.last is not None:
        assert torch.equal(st.last, dev(led.last)), what
    if st.last_len is not None:
        assert torch.equal(st.last_len, dev(led.last_len)), what
    got, want = st.totals.cpu().numpy(), led.totals
    assert (got[:, 2 + 4 * C:] == POISON).all(), what                                      # the padding is untouched
    exact = [0, 1] + [4 + 4 * c for c in range(C)] + [5 + 4 * c for c in range(C)]
    assert np.array_equal(got[:, exact], want[:, exact]), what
    worst = 0.0
    for m in range(st.K):
        b_sum, b_sq = model.sum_bounds(led.episodes[m], C, None if prior is None else prior[m])
        for c in range(C):
            for slot, bound in ((2 + 4 * c, b_sum[c]), (3 + 4 * c, b_sq[c])):
                err = abs(got[m, slot] - want[m, slot])
                assert err <= bound, (what, m, c, slot, err, bound)
                if bound > 0:
                    worst = max(worst, err / bound)
        if not led.episodes[m] and prior is None:
            assert not got[m, :2 + 4 * C].any(), (what, m)
    print("episode ledger %s: largest error / bound = %.3g" % (what, worst))
    return worst


# ---------------------------------------------------------------------------------------------- synthetic rows, the library
@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.05, 0.5, 1.0])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_ledger_against_the_model(shape, p):
    """Two successive calls (the second merges into rows that hold episodes), each against the model; and the same two calls
    again: the same bits."""
    T, N, K, C = shape
    st, again, led = _State(N, K, C), _State(N, K, C), _model(N, K, C)
    for call in range(2):
        reward, done, steps = _inputs(T + call, N, p, 1000 * call + T + N + int(100 * p))
        steps = steps if C > 1 else None
        led.update(reward, done, steps)
        st.update(reward, done, steps)
        again.update(reward, done, steps)
        _check(st, led, (shape, p, call))
        for a, b in zip(st.tensors(), again.tensors()):
            assert torch.equal(a, b), (shape, p, call)
    assert int(st.totals[:, 0].sum()) == int(sum(len(e) for e in led.episodes))


@pytest.mark.gpu
def test_an_episode_length_of_400_with_done_at_the_last_step():
    T, N, K, C = 400, 130, 2, 2
    reward, _, steps = _inputs(T, N, 0.0, 400)
    done = np.zeros((T, N), dtype=np.uint8)
    done[T - 1] = 1
    st, led = _State(N, K, C), _model(N, K, C)
    led.update(reward, done, steps)
    st.update(reward, done, steps)
    _check(st, led, "400 steps")
    assert st.totals[:, 0].tolist() == [65.0, 65.0] and st.totals[:, 1].tolist() == [65.0 * 400, 65.0 * 400]
    assert bool((st.last_len == 400).all()) and not bool(st.carry.any()) and not bool(st.carry_len.any())


@pytest.mark.gpu
def test_episodes_ending_at_the_first_and_the_last_step():
    T, N, K, C = 5, 63, 1, 2
    reward, _, steps = _inputs(T, N, 0.0, 11)
    done = np.zeros((T, N), dtype=np.uint8)
    done[0, ::2] = 1
    done[T - 1, 1::3] = 1
    st, led = _State(N, K, C), _model(N, K, C)
    led.update(reward, done, steps)
    st.update(reward, done, steps)
    _check(st, led, "first and last step")
    lens = st.last_len.tolist()
    assert lens[0] == 1 and lens[1] == T and lens[4] == T - 1 and lens[5] == 0     # env 4: both ends; env 5: neither
    assert st.carry_len.tolist()[0] == T - 1 and st.carry_len.tolist()[1] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("filled", [False, True])
def test_a_member_without_a_finished_episode_keeps_its_row(filled):
    T, K, n_m, C = 6, 3, 65, 3
    N = K * n_m
    reward, done, steps = _inputs(T, N, 0.3, 21)
    done[:, n_m:2 * n_m] = 0                                     # member 1 finishes nothing
    st, led = _State(N, K, C), _model(N, K, C)
    prior = None
    if filled:                                                   # rows that hold episodes on entry: {2, 9, per channel 1, 5, -2, 3}
        row = np.array([2.0, 9.0] + [1.0, 5.0, -2.0, 3.0] * C)
        led.totals[:, :2 + 4 * C] = row
        st.totals[:, :2 + 4 * C] = torch.from_numpy(row).to(DEV)
        prior = [row] * K
    before = st.totals[1].clone()
    led.update(reward, done, steps)
    st.update(reward, done, steps)
    _check(st, led, ("no episode", filled), prior)
    assert torch.equal(st.totals[1], before)
    assert float(st.totals[0, 0]) > (2.0 if filled else 0.0) and float(st.totals[2, 0]) > (2.0 if filled else 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(9, 6 * 65, 6, 8), (7, 257, 1, 3)], ids=IDS)
def test_two_calls_over_a_split_equal_one_call(shape):
    T, N, K, C = shape
    reward, done, steps = _inputs(T, N, 0.2, 31)
    one = _State(N, K, C)
    one.update(reward, done, steps)
    exact = [0, 1] + [4 + 4 * c for c in range(C)] + [5 + 4 * c for c in range(C)]
    for T1 in (1, 4, T - 1):
        two = _State(N, K, C)
        two.update(reward[:T1], done[:T1], steps[:T1])
        two.update(reward[T1:], done[T1:], steps[T1:])
        for name in ("carry", "carry_len", "last", "last_len"):
            assert torch.equal(getattr(one, name), getattr(two, name)), (shape, T1, name)
        assert torch.equal(one.totals[:, exact], two.totals[:, exact]), (shape, T1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(9, 6 * 65, 6, 8), (5, 3 * 300, 3, 3), (4, 1024, 1024, 2)], ids=IDS)
def test_members_equal_stand_alone_calls(shape):
    """Every buffer of a member, the totals row included: bit-equal to the stand-alone entry point on a contiguous copy of its
    columns -- after two calls, so that the second merges into a row that holds episodes."""
    T, N, K, C = shape
    n_m = N // K
    members = range(K) if K <= 8 else (0, 1, 511, 1023)
    pop = _State(N, K, C)
    alone = {m: _State(n_m, 1, C) for m in members}
    for call in range(2):
        reward, done, steps = _inputs(T + call, N, 0.4, 41 + call)
        pop.update(reward, done, steps)
        for m, st in alone.items():
            lo, hi = m * n_m, (m + 1) * n_m
            st.update(np.ascontiguousarray(reward[:, lo:hi]), np.ascontiguousarray(done[:, lo:hi]), np.ascontiguousarray(steps[:, lo:hi]),
                      alone=True)
    for m, st in alone.items():
        lo, hi = m * n_m, (m + 1) * n_m
        for name in ("carry", "carry_len", "last", "last_len"):
            assert torch.equal(getattr(pop, name)[lo:hi], getattr(st, name)), (shape, m, name)
        assert torch.equal(pop.totals[m], st.totals[0]), (shape, m)
    assert float(pop.totals[:, 0].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("last,last_len", [(False, False), (True, False), (False, True)])
def test_last_may_be_null(last, last_len):
    T, N, K, C = 7, 257, 1, 3
    reward, done, steps = _inputs(T, N, 0.3, 51)
    st, led = _State(N, K, C, last=last, last_len=last_len), _model(N, K, C)
    led.update(reward, done, steps)
    st.update(reward, done, steps)
    _check(st, led, ("NULL", last, last_len))


@pytest.mark.gpu
def test_rewards_alone_need_no_step_records():
    """C == 1 with steps == NULL and cols == NULL: the same buffers as with step records that are not read."""
    T, N, K = 5, 63, 1
    reward, done, steps = _inputs(T, N, 0.3, 61)
    a, b, led = _State(N, K, 1), _State(N, K, 1), _model(N, K, 1)
    led.update(reward, done)
    a.update(reward, done, None)
    b.update(reward, done, steps)
    _check(a, led, "steps == NULL")
    for x, y in zip(a.tensors(), b.tensors()):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------- with the env
@pytest.mark.gpu
@pytest.mark.parametrize("staggered", [False, True])
def test_last_reproduces_the_envs_own_episode_returns(staggered):
    """192 envs of 12-step episodes, 30 steps by step_many in chunks of 7 under fixed random actions, in lockstep and -- after 5
    steps and a masked reset of every third env, before the ledger starts -- staggered: the ledger's reward-column channel of
    every env's last finished episode is the env's own last_return, bit for bit."""
    N, L, total = 192, 12, 30
    env = pcc_rl_amd.BatchedNetworkEnv(N, device=DEV, seed=5, max_steps=L)
    env.reset()
    g = torch.Generator(device="cpu").manual_seed(8)
    actions = torch.randn((5 + total, N), generator=g).to(DEV)
    if staggered:
        env.step_many(actions[:5])
        env.reset(mask=torch.arange(N) % 3 == 0)
    ledger = EpisodeLedger(N, channels=("reward", "sent"), device=DEV)
    assert ledger.names == ["reward_f32", "reward", "sent"]
    n_done = 0
    for t0 in range(0, total, 7):
        n = min(7, total - t0)
        rew = torch.empty((n, N), device=DEV)
        done = torch.empty((n, N), dtype=torch.uint8, device=DEV)
        steps = torch.empty((n, N, 19), dtype=torch.float64, device=DEV)
        env.step_many(actions[5 + t0:5 + t0 + n], reward_out=rew, done_out=done, steps_out=steps)
        ledger.update(rew, done, steps)
        n_done += int(done.sum())
    env.check_flags()
    finished = ledger.last_len > 0
    assert bool(finished.all())                                                    # (30 steps: every env finished one)
    assert torch.equal(ledger.last[:, 1], env.episode_returns())
    assert bool((ledger.last_len == L).all())
    if staggered:                                                                  # (the done rows were staggered indeed)
        assert not torch.equal(ledger.carry_len[0], ledger.carry_len[1])
    assert int(ledger.totals()[0, 0]) == n_done == 2 * N                           # (either way two episode ends per env)
    s = ledger.summary()
    assert s["episodes"] == [n_done] and s["mean_length"][0] == (L if not staggered else (N * 2 * L - (N - N // 3) * 5) / (2.0 * N))
    env.close()


# ------------------------------------------------------------------------------------------------------------ the trainers
N_T, H_T, L_T = 512, 16, 24   # envs, horizon, episode length: the second rollout finishes every env's episode at its step 7


def _trainer_env(seed=3):
    return pcc_rl_amd.BatchedNetworkEnv(N_T, device=DEV, seed=seed, max_steps=L_T, ring_pools=POOLS)


def _spy(agent):
    """Record the rows every ledger update of `agent` is fed."""
    fed, inner = [], agent.ledger.update

    def update(rew, done, steps=None):
        fed.append((rew.cpu().numpy().copy(), done.cpu().numpy().astype(np.uint8)))
        return inner(rew, done, steps)
    agent.ledger.update = update
    return fed


def _same_stat(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _check_iteration(stats, new, members):
    """iterate()'s episodes / mean_episode_return / mean_episode_length against the model's episodes of that rollout, per member:
    counts and lengths exact, the mean return within the sum bound over E (the totals before this rollout held no episode: the
    difference is the rollout's own sum)."""
    eps, ret, length = stats["episodes"], stats["mean_episode_return"], stats["mean_episode_length"]
    if members == 1:
        eps, ret, length = [eps], [ret], [length]
    for m in range(members):
        E = len(new[m])
        assert eps[m] == E
        if E == 0:
            assert math.isnan(ret[m]) and math.isnan(length[m])
            continue
        v = [float(e[2][0]) for e in new[m]]
        bound = model.sum_bounds(new[m], 1)[0][0] / E
        assert abs(ret[m] - math.fsum(v) / E) <= bound + 2.0 ** -52 * abs(ret[m]), (m, ret[m], math.fsum(v) / E, bound)
        assert length[m] == sum(e[1] for e in new[m]) / E


@pytest.mark.gpu
@pytest.mark.parametrize("option", [{}, {"policy_in_step": True}, {"normalize_obs": True}], ids=["fused", "policy_in_step", "normalize_obs"])
def test_ppo_reports_the_models_episodes_and_trains_as_without(option):
    env_a, env_b = _trainer_env(), _trainer_env()
    a = PPO(env_a, horizon=H_T, seed=1, track_episodes=True, **option)
    b = PPO(env_b, horizon=H_T, seed=1, **option)
    fed, led = _spy(a), model.Ledger(N_T)
    for it in range(2):
        torch.manual_seed(100 + it)
        stats = a.iterate()
        torch.manual_seed(100 + it)
        plain = b.iterate()
        assert sorted(set(stats) - set(plain)) == ["episodes", "mean_episode_length", "mean_episode_return"]
        assert all(_same_stat(stats[k], plain[k]) for k in plain)
        rew, done = fed[it]
        assert rew.shape == (H_T, N_T) and done.sum() == (N_T if it == 1 else 0) and (it == 0 or done[L_T - H_T - 1].all())
        _check_iteration(stats, led.update(rew, done), 1)
        assert stats["episodes"] == (N_T if it == 1 else 0)
    assert stats["mean_episode_length"] == L_T
    assert torch.equal(a.flat, b.flat) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.obs, b.obs)
    # ... and the ledger's own buffers are the model's
    assert torch.equal(a.ledger.carry, torch.from_numpy(led.carry).to(DEV)) and torch.equal(a.ledger.last, torch.from_numpy(led.last).to(DEV))
    assert bool((a.ledger.last_len == L_T).all()) and bool((a.ledger.carry_len == 2 * H_T - L_T).all())
    env_a.close(); env_b.close()


@pytest.mark.gpu
def test_ppo_checkpoint_carries_the_ledger():
    env_a, env_b, env_c = _trainer_env(), _trainer_env(), _trainer_env()
    a = PPO(env_a, horizon=H_T, seed=1, track_episodes=True)
    a.iterate()
    sd = a.state_dict()
    assert sd["track_episodes"] is True and sorted(sd["episodes"]) == ["carry", "carry_len", "columns", "last", "last_len", "members", "n_envs", "totals"]
    assert bool((sd["episodes"]["carry_len"] == H_T).all())
    want = a.iterate()
    b = PPO(env_b, horizon=H_T, seed=9, track_episodes=True)                  # (another start: everything comes from the state)
    b.load_state_dict(sd)
    got = b.iterate()
    assert got["episodes"] == N_T and sorted(got) == sorted(want) and all(_same_stat(got[k], want[k]) for k in want)
    for name in ("carry", "carry_len", "last", "last_len"):
        assert torch.equal(getattr(a.ledger, name), getattr(b.ledger, name)), name
    assert torch.equal(a.ledger.totals(), b.ledger.totals()) and torch.equal(a.flat, b.flat)
    c = PPO(env_c, horizon=H_T, seed=1)
    with pytest.raises(ValueError, match="track_episodes=True, this object has track_episodes=False"):
        c.load_state_dict(sd)
    with pytest.raises(ValueError, match="track_episodes=False, this object has track_episodes=True"):
        b.load_state_dict(c.state_dict())
    assert "track_episodes" not in c.state_dict() and "episodes" not in c.state_dict()
    bad = dict(sd, episodes=dict(sd["episodes"], n_envs=N_T // 2))
    with pytest.raises(ValueError, match="episode ledger is of another shape"):
        b.load_state_dict(bad)
    env_a.close(); env_b.close(); env_c.close()


KP = 4


def _population_run(spy=False):
    """A population of 4 on 512 envs, two iterations from fixed seeds of the device's generator; between them member 2's envs are
    reset, so that its episodes -- 16 steps behind the others' from there -- do not finish in the second rollout."""
    env = _trainer_env(seed=21)
    pop = PopulationPPO(env, KP, horizon=H_T, seeds=[0, 1, 2, 3], lr=[1e-3, 3e-4, 1e-4, 3e-5], track_episodes=True)
    fed = _spy(pop) if spy else None
    stats = []
    n_m = N_T // KP
    for it in range(2):
        torch.manual_seed(60 + it)                               # (the noise and the permutations: the device's generator)
        stats.append(pop.iterate())
        if it == 0:
            mask = (torch.arange(N_T) // n_m) == 2
            pop.obs[2 * n_m:3 * n_m] = env.reset(mask=mask)[2 * n_m:3 * n_m]
    return env, pop, stats, fed


@pytest.mark.gpu
def test_population_reports_per_member_and_evolves_on_the_ledger():
    env_a, a, stats, fed = _population_run(spy=True)
    led = model.Ledger(N_T, KP)
    _check_iteration(stats[0], led.update(*fed[0]), KP)
    assert stats[0]["episodes"] == [0] * KP
    new = led.update(*fed[1])
    assert [len(e) for e in new] == [128, 128, 0, 128]
    _check_iteration(stats[1], new, KP)
    assert sorted(stats[1]) == ["clip_frac", "entropy", "episodes", "mean_episode_length", "mean_episode_return", "mean_step_reward", "pg", "vf"]
    scores = a.ledger.scores().clone()
    assert math.isnan(scores.tolist()[2]) and all(math.isfinite(x) for i, x in enumerate(scores.tolist()) if i != 2)
    want = [math.fsum(float(e[2][0]) for e in new[m]) / 128 for m in (0, 1, 3)]
    assert all(abs(scores.tolist()[m] - w) <= model.sum_bounds(new[m], 1)[0][0] / 128 for m, w in zip((0, 1, 3), want))
    env_b, b, _, _ = _population_run()
    assert torch.equal(a.flat, b.flat) and torch.equal(a.ledger.totals(), b.ledger.totals())
    with pytest.raises(ValueError, match="track_episodes=True"):
        PopulationPPO.evolve(type("P", (), {"track_episodes": False, "env": env_a, "members": KP})(), None)
    before = b.ledger.totals().clone()
    pa, ra = a.evolve(frac=0.25, seed=5)                       # scores=None: the ledger's
    pb, rb = b.evolve(scores, frac=0.25, seed=5)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ra, rb)
    for name in ("flat", "adam_m", "adam_v", "hyper"):
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
    # the member without a finished episode ranks last and is replaced; its row and only its row is cleared where the scores
    # were passed, every row where the ledger's own were taken
    parent = pa.tolist()
    assert ra.tolist()[2] == KP - 1 and parent[2] != 2 and [parent[m] for m in (0, 1, 3)] == [0, 1, 3]
    assert not bool(a.ledger.totals().any())
    assert not bool(b.ledger.totals()[2].any()) and torch.equal(b.ledger.totals()[[0, 1, 3]], before[[0, 1, 3]])
    assert bool(a.ledger.carry_len.any()) and torch.equal(a.ledger.carry, b.ledger.carry)       # the running episodes go on
    # a replaced member that had episodes: its row is cleared, the others stay
    b.ledger.totals().copy_(before)
    b.ledger.totals()[2] = before[0]
    p2, _ = b.evolve([3.0, 0.0, 2.0, 1.0], frac=0.25, seed=6)
    assert p2.tolist()[1] == 0 and not bool(b.ledger.totals()[1].any()) and torch.equal(b.ledger.totals()[[0, 2, 3]], before[[0, 0, 3]])
    sd = b.state_dict()
    assert sd["track_episodes"] is True and torch.equal(sd["episodes"]["totals"], b.ledger.totals())
    env_a.close(); env_b.close()


# -------------------------------------------------------------------------------------------------------------- evaluate
@pytest.mark.gpu
def test_evaluate_reports_the_envs_own_returns(monkeypatch):
    """256 envs, one episode of 40 steps under the zero action, in chunks of 7 steps: 256 episodes, every env's reward-column total
    the env's own last_return bit for bit, their mean within the sum bound of the exactly rounded mean."""
    N, L = 256, 40
    monkeypatch.setattr(evaluate_module, "STEPS_BYTES", 7 * N * 19 * 8 + 1)
    env = pcc_rl_amd.BatchedNetworkEnv(N, device=DEV, seed=12, max_steps=L)
    seen = []

    def zero(obs_row, out_act_row):
        assert obs_row.shape == (N, env.obs_dim) and out_act_row.shape == (N,)
        out_act_row.zero_()
    out = evaluate(env, zero, channels=("reward", "sent", "acked", "lost", "run_dur", "latency_ratio"),
                   step_hook=lambda t, row: seen.append((t, tuple(row.shape))))
    assert seen == [(t, (N, 19)) for t in range(L)]
    assert out["episodes"] == [N] and out["mean_length"] == [float(L)]
    returns = env.episode_returns()
    assert torch.equal(out["last"][:, 1], returns) and bool((out["last_len"] == L).all())
    v = returns.tolist()
    bound = N * 2.0 ** -52 * math.fsum(abs(x) for x in v) / N
    assert abs(out["channels"]["reward"]["mean"][0] - math.fsum(v) / N) <= bound
    assert abs(out["channels"]["reward"]["mean"][0] - float(returns.mean())) <= 2 * bound      # (torch's own mean: as far again)
    sent, lost = out["last"][:, 2], out["last"][:, 4]
    assert abs(out["loss_ratio"][0] - float(lost.sum() / sent.sum())) <= 1e-12
    assert abs(out["mean_latency_ratio"][0] - float(out["last"][:, 6].sum()) / (N * L)) <= 1e-9 * out["mean_latency_ratio"][0]
    assert out["channels"]["sent"]["min"][0] == float(sent.min()) and out["channels"]["sent"]["max"][0] == float(sent.max())
    with pytest.raises(ValueError, match="episodes"):
        evaluate(env, zero, episodes=0)
    env.close()
