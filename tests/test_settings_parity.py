"""GPU parity with the handle's own settings moved off their defaults: delta_scale (once per place where the device restates
"scale the action, move the rate or window, clamp"), the sampling ranges of pcc_set_param_ranges, a new seed / new ranges / arrays
and back while the envs are out of lockstep, and actions that are infinite or overflow.  Everything is np.array_equal or
torch.equal -- the 19 step columns, observations against the float32 cast of the oracle's, dones, the state fields a test names --
and every env ends with check_flags() clean.  The reference side of every comparison is checked by itself, on the CPU, in
tests/test_oracle_settings_cpu.py (the range sets and action helpers come from there)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import oracle
import pcc_rl_amd
from pcc_rl_amd import native
from test_gpu_parity import DEV, run_gpu
from test_oracle_settings_cpu import RANGE_SETS, actions, extreme_rate_actions
from test_rollout import _buffers, _compare, _make, _params, _small_batches

pytestmark = pytest.mark.gpu
Env = pcc_rl_amd.BatchedNetworkEnv


def same_as_oracle(got, ref, obs0=None, what=""):
    """got = run_gpu()'s (steps, obs, dones) of an episode shorter than max_steps; ref = oracle.run_batch()'s dict."""
    steps, obs, done = got
    if obs0 is not None:
        assert np.array_equal(obs0.reshape(ref["obs0"].shape), ref["obs0"].astype(np.float32)), what
    bad = np.argwhere((steps[..., :3] != ref["steps"][..., :3]).any(axis=tuple(range(1, steps.ndim))))
    assert bad.size == 0, (what, "envs with count mismatches: %s" % bad[:10].ravel())
    assert np.array_equal(steps, ref["steps"]), what
    assert np.array_equal(obs.reshape(ref["obs"].shape), ref["obs"].astype(np.float32)), what
    assert not done.any(), what


def oracle_envs(n, seed, n_senders=1, delta_scale=0.025, cwnd=False):
    out = []
    for i in range(n):
        o = oracle.OracleEnv(n_senders, delta_scale=delta_scale)
        o.rng_philox(seed, i)
        if cwnd:
            o.use_cwnd(True)
        out.append(o)
    return out


def step_against_oracle_envs(env, oenvs, a, osteps, max_steps, t, cwnd=False):
    """One step of every env against its own oracle object (the per-env loop of tests/test_gpu_parity.py's out-of-lockstep tests):
    the 19 columns of every sender, done, the observation (after an auto-reset: the next episode's first), with `cwnd` the windows."""
    n, S = env.n_envs, env.n_senders
    o_gpu, r_gpu, d_gpu, info = env.step(torch.as_tensor(a, dtype=torch.float64, device=DEV))
    rows = info["steps"].cpu().numpy().reshape(n, S, native.PCC_STEP_COLS)
    o_gpu, d_gpu = o_gpu.cpu().numpy().reshape(n, S, -1), d_gpu.cpu().numpy()
    cw = env.state("cwnd").cpu().numpy() if cwnd else None
    for i in range(n):
        o_ref, _, _, _ = oenvs[i].step(a[i])
        osteps[i] += 1
        done = osteps[i] >= max_steps
        assert np.array_equal(rows[i], oenvs[i].last_row), (t, i)
        if cwnd:
            assert [int(cw[s, i]) for s in range(S)] == [oenvs[i].cwnd(s) for s in range(S)], (t, i)
        assert bool(d_gpu[i]) == done, (t, i)
        if done and env.auto_reset:
            o_ref = oenvs[i].reset()
            osteps[i] = 0
        assert np.array_equal(o_gpu[i], np.asarray(o_ref).reshape(S, -1).astype(np.float32)), (t, i)


# ---------------------------------------------------------------------------------------------------------------- 2. delta_scale
# one entry per place that scales an action: name -> (env arguments, tuning knobs, how it is stepped, envs, steps)
# (the event loop runs an interval packet by packet: its cases are the small ones)
RATE_PATHS = {
    # apply_rate_delta (pcc_dev.h) under the one-sender work lists: lane rounds and wave passes by default, every env on the wave
    # path, every env a team item
    "lists": (dict(), dict(), "step", 384, 40),
    "lists_wave": (dict(), dict(heavy_predict=0.0), "step", 384, 40),
    "lists_team": (dict(), dict(heavy_predict=0.0, team_predict=0.0), "step", 384, 40),
    # ... in the small-batch kernel, the steps up to the episode's end in one launch
    "small_step_many": (dict(), None, "step_many", 384, 40),
    # ... with two senders
    "lists_two_senders": (dict(n_senders=2), dict(), "step", 384, 40),
    # latency noise: one sender by sorting (1), the small instance crossed with the event loop (2), the event loop (0) -- the first
    # two run noise_sorted_kernel's copy; two senders by sorting (noise_sorted2_kernel's copy) and by the event loop
    "noise_sorted1": (dict(latency_noise=1.1), dict(noise_sorted=1), "step", 384, 40),
    "noise_sorted2": (dict(latency_noise=1.1), dict(noise_sorted=2), "step", 320, 32),
    "noise_sorted0": (dict(latency_noise=1.1), dict(noise_sorted=0), "step", 320, 32),
    "noise_two_senders_sorted1": (dict(latency_noise=1.1, n_senders=2), dict(noise_sorted=1), "step", 384, 40),
    "noise_two_senders_sorted0": (dict(latency_noise=1.1, n_senders=2), dict(noise_sorted=0), "step", 256, 30),
}


@pytest.mark.parametrize("scale", [0.2, 1.0])
@pytest.mark.parametrize("path", sorted(RATE_PATHS))
def test_delta_scale_reaches_every_rate_path(path, scale):
    """delta_scale = 0.2 and 1.0 (the reference's 0.025 is the only value the other files use) through every path that applies a
    rate action, actions U(-1, 1.5): a copy that read a constant, or that scaled before its NaN test, differs from the oracle in
    the rate column of the first step."""
    kw, knobs, how, n, T = RATE_PATHS[path]
    seed = 5
    S = kw.get("n_senders", 1)
    if knobs is None:
        Env.DEFAULT_LIST_MIN_ENVS = None      # (the conftest's fixture puts its 0 back)
    acts = actions(seed, n, T, S)
    ref = oracle.run_batch(acts, n_senders=S, seed=seed, delta_scale=scale, latency_noise=kw.get("latency_noise"))
    env = Env(n, device=DEV, seed=seed, record_steps=True, auto_reset=how == "step_many", delta_scale=scale, **kw)
    env.set_tuning(**(knobs or {}))
    obs0 = env.reset().cpu().numpy()
    if how == "step":
        got = run_gpu(env, acts, T)
    else:
        a = torch.as_tensor(np.ascontiguousarray(np.moveaxis(acts, 1, 0)), dtype=torch.float64, device=DEV)
        obs = torch.empty((T, n, S, env.obs_dim), device=DEV)
        rew = torch.empty((T, n, S), device=DEV)
        done = torch.empty((T, n), dtype=torch.uint8, device=DEV)
        rows = torch.empty((T, n, S, native.PCC_STEP_COLS), dtype=torch.float64, device=DEV)
        env.step_many(a, obs, rew, done, rows)
        torch.cuda.synchronize()
        env.check_flags()
        got = (rows[:, :, 0].transpose(0, 1).cpu().numpy(), obs[:, :, 0].transpose(0, 1).cpu().numpy(), done.t().cpu().numpy() != 0)
    same_as_oracle(got, ref, obs0, (path, scale))
    # (the scale is in the comparison: the reference's own gives other rates on the same actions)
    plain = oracle.run_batch(acts[:, :2], n_senders=S, seed=seed, latency_noise=kw.get("latency_noise"), want_obs=False)
    assert not np.array_equal(plain["steps"][..., 3], ref["steps"][..., :2, 3])
    env.close()


def test_rate_jumps_between_floor_and_ceiling_at_delta_scale_one():
    """Actions of +-30 at delta_scale = 1.0 on the one-sender work-list path: x 31 or / 31 a step, so the rate jumps between
    MIN_RATE and MAX_RATE in a single step, again and again -- every prediction the retire half files for the next send half is
    off by a factor of 25 half of the time, and rings are promoted for a load that is gone one step later.  No flag, every column."""
    n, T, seed = 512, 60, 6
    acts = np.random.RandomState(seed).choice([-30.0, 30.0], (n, T))
    ref = oracle.run_batch(acts, seed=seed, delta_scale=1.0)
    rate = ref["steps"][..., 3]
    # (rate0 * 31 can stay below the ceiling at the first step; from the second on it is one or the other)
    assert np.isin(rate[:, 1:], (40.0, 1000.0)).all() and (rate == 40.0).any() and (rate == 1000.0).any()
    env = Env(n, device=DEV, seed=seed, record_steps=True, auto_reset=False, delta_scale=1.0)
    obs0 = env.reset().cpu().numpy()
    same_as_oracle(run_gpu(env, acts, T), ref, obs0)
    env.close()


@pytest.mark.parametrize("scale", [0.2, 1.0])
@pytest.mark.parametrize("n_senders", [1, 2])
def test_delta_scale_reaches_the_window(n_senders, scale):
    """use_cwnd with one sender (the send half's own copy of apply_cwnd_delta, pcc_send_item.h) and with two (the event-loop build,
    the helper of pcc_dev.h): rate and window actions U(-1, 1.5), every env against its own oracle object, the window after every
    step."""
    n, T, seed = 256, 30, 7
    env = Env(n, device=DEV, seed=seed, n_senders=n_senders, record_steps=True, auto_reset=False, use_cwnd=True, delta_scale=scale)
    oenvs = oracle_envs(n, seed, n_senders, scale, cwnd=True)
    obs0 = env.reset().cpu().numpy()
    assert np.array_equal(obs0.reshape(n, n_senders, -1), np.stack([np.asarray(o.reset()).reshape(n_senders, -1) for o in oenvs]).astype(np.float32))
    acts = np.random.RandomState(seed).uniform(-1, 1.5, (n, T, n_senders, 2))
    osteps = np.zeros(n, dtype=int)
    windows = set()
    for t in range(T):
        step_against_oracle_envs(env, oenvs, acts[:, t], osteps, 400, t, cwnd=True)
        windows.update(o.cwnd(0) for o in oenvs[:16])
    assert len(windows) > 16      # (the windows do move)
    env.check_flags()
    env.close()


def test_rollout_equals_the_loop_at_another_delta_scale(monkeypatch):
    """pcc_rollout's contract (rollout == policy kernel + pcc_step, tests/test_rollout.py) on handles with delta_scale = 0.2: the
    policy in the retire launch's epilogue at 3 000 envs, the smallest batch that file runs with work lists, and in the small-batch
    kernel's loop; the latter also tied to the oracle, fed the actions the rollout took."""
    _compare(lambda: _make(3000, 31, delta_scale=0.2, max_steps=25), 40)
    _small_batches(monkeypatch)
    _compare(lambda: _make(1000, 32, delta_scale=0.2, max_steps=25), 40)
    n, T, seed = 512, 30, 33
    env = Env(n, device=DEV, seed=seed, auto_reset=False, delta_scale=0.2)
    env.reset()
    b = _buffers(env, T)
    b["obs"][0].copy_(env._obs)
    noise = torch.randn((T, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    env.rollout(_params(env.obs_dim), noise, b["obs"], b["act"], None, None, None, None, b["steps"])
    env.check_flags()
    ref = oracle.run_batch(b["act"][:, :, 0].t().double().cpu().numpy(), seed=seed, delta_scale=0.2)
    assert np.array_equal(b["steps"][:, :, 0].transpose(0, 1).cpu().numpy(), ref["steps"])
    assert np.array_equal(b["obs"][1:, :, 0].transpose(0, 1).cpu().numpy(), ref["obs"].astype(np.float32))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 3. parameter ranges
@pytest.mark.parametrize("n_senders", [1, 2])
@pytest.mark.parametrize("name", sorted(RANGE_SETS))
def test_parameter_ranges_match_oracle(name, n_senders):
    """randomize_link_params(ranges) against the oracle with the same ranges: the links the reset drew -- the queue too, as
    maxq = (1 + floor(e^x)) / bw -- then every column of 36 steps.  The sets and the edge each is there for:
    tests/test_oracle_settings_cpu.py."""
    n, T, seed = 320, 36, 13
    lo, hi = RANGE_SETS[name]
    S = n_senders
    acts = actions(seed, n, T, S)
    if name == "every_packet_lost":
        acts = np.ascontiguousarray(np.broadcast_to(acts[:1], acts.shape))      # one link, no draw that matters: one env, n times
    ref = oracle.run_batch(acts, n_senders=S, seed=seed, ranges=(lo, hi))
    env = Env(n, device=DEV, seed=seed, n_senders=S, record_steps=True, auto_reset=False)
    env.randomize_link_params((lo, hi))
    obs0 = env.reset().cpu().numpy()
    p = ref["params"]
    queue = np.round(p[:, 2])      # (the oracle reports max_queue_delay * bw: the integer up to rounding)
    assert (queue >= 1 + math.floor(math.exp(lo[2]))).all() and (queue <= 1 + math.floor(math.exp(hi[2]))).all()
    state = lambda f: env.state(f).cpu().numpy()
    assert np.array_equal(state("bw"), p[:, 0])
    assert np.array_equal(state("dl"), p[:, 1])
    assert np.array_equal(state("lr"), p[:, 3])
    assert np.array_equal(state("rate0"), p[:, 4:4 + S].T)
    assert np.array_equal(state("maxq"), queue / p[:, 0])
    got = run_gpu(env, acts, T)
    same_as_oracle(got, ref, obs0, name)
    steps = got[0]
    if name == "every_packet_lost":
        # every env is the same env, and the same as a handle given the constants as arrays: no oracle in this
        assert (steps == steps[:1]).all() and (steps[..., 1] == 0).all() and steps[..., 2].sum() > 0
        twin = Env(n, device=DEV, seed=seed + 1, n_senders=S, record_steps=True, auto_reset=False)
        twin.set_link_params(lo[0], lo[1], 1.0 + math.floor(math.exp(lo[2])), lo[3], lo[4] * lo[0])
        obs0_t = twin.reset().cpu().numpy()
        got_t = run_gpu(twin, acts, T)
        assert np.array_equal(obs0, obs0_t) and all(np.array_equal(x, y) for x, y in zip(got, got_t))
        twin.close()
    if name == "default_explicit":
        twin = Env(n, device=DEV, seed=seed, n_senders=S, record_steps=True, auto_reset=False)      # never called the setter
        obs0_t = twin.reset().cpu().numpy()
        got_t = run_gpu(twin, acts, T)
        assert np.array_equal(obs0, obs0_t) and all(np.array_equal(x, y) for x, y in zip(got, got_t))
        twin.close()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 4. out of lockstep
SEED2 = (0x9E3779B9 << 32) | 20240607      # a non-zero high word: key1


@pytest.mark.parametrize("change", ["seed", "ranges", "ranges_c_abi", "arrays_and_back"])
def test_source_of_the_next_episode_changes_out_of_lockstep(change):
    """The schedule of test_new_link_params_out_of_lockstep_apply_at_every_envs_next_reset (96 envs, episodes of 20 steps, masked
    resets that stagger them, a change at step 33, two more episodes) with the other three things that move params_gen: a new
    seed -- the oracle keys every draw by (index, interval, episode, env id) under the key, so the running episode's loss draws
    switch key at that step and every next episode is drawn under the new one --, new sampling ranges -- running episodes go on,
    every env's next reset draws from them (through randomize_link_params, and through pcc_set_param_ranges alone) --, and link arrays followed, a little later, by sampling again.  An episode prepared
    ahead of time under the old key, ranges or arrays must not be swapped in; and shadows must come back into use afterwards."""
    n, seed, max_steps, T, t_change, t_back = 96, 19, 20, 100, 33, 58
    env = Env(n, device=DEV, seed=seed, record_steps=True, auto_reset=True, max_steps=max_steps)
    oenvs = oracle_envs(n, seed)
    obs = env.reset().cpu().numpy()
    assert np.array_equal(obs, np.stack([o.reset() for o in oenvs]).astype(np.float32))
    osteps = np.zeros(n, dtype=int)
    rs = np.random.RandomState(8)
    idx = np.arange(n)
    lo, hi = RANGE_SETS["slow_lossy_shallow"]
    new = dict(bw=150.0 + idx, dl=0.04 + 0.001 * idx, queue=5.0 + (idx % 40), loss=0.002 * (idx % 10), rate0=90.0 + 2.0 * idx)
    swaps = {}
    for t in range(T):
        if t < 20 and t % 5 == 2:      # stagger the episode phases (masked resets), so that shadows come into use
            mask = (idx % 4) == ((t // 5) % 4)
            got = env.reset(torch.as_tensor(mask)).cpu().numpy()
            for i in idx[mask]:
                want = oenvs[i].reset()
                osteps[i] = 0
                assert np.array_equal(got[i], want.astype(np.float32)), (t, i)
        if t == t_change:
            swaps["before"] = env.restart_stats()["shadow_swaps"]
            if change == "seed":
                assert env.seed(SEED2) == [SEED2]
                for i in range(n):
                    oenvs[i].rng_philox(SEED2, i)
            elif change.startswith("ranges"):
                if change == "ranges":
                    env.randomize_link_params((lo, hi))
                else:      # pcc_set_param_ranges alone (randomize_link_params calls pcc_set_link_params first, a setter of its own)
                    dbl5 = ctypes.c_double * 5
                    native.check(env._L.pcc_set_param_ranges(env._h, dbl5(*lo), dbl5(*hi)))
                for o in oenvs:
                    o.set_ranges(lo, hi)
            else:
                env.set_link_params(new["bw"], new["dl"], new["queue"], new["loss"], new["rate0"])
                for i in range(n):
                    oenvs[i].set_params(new["bw"][i], new["dl"][i], new["queue"][i], new["loss"][i], [new["rate0"][i]])
        if t == t_back and change == "arrays_and_back":
            assert np.array_equal(env.state("bw").cpu().numpy(), new["bw"])      # (every env has restarted on its array link)
            env.randomize_link_params()
            for o in oenvs:
                o.clear_params()
        step_against_oracle_envs(env, oenvs, rs.uniform(-1, 1.2, n), osteps, max_steps, t)
        if t == t_change or (t == t_back and change == "arrays_and_back"):
            swaps["at_last_change"] = env.restart_stats()["shadow_swaps"]      # (after the first step that follows it)
    swaps["end"] = env.restart_stats()["shadow_swaps"]
    print("shadow swaps (%s): %s" % (change, swaps))
    bw = env.state("bw").cpu().numpy()
    if change.startswith("ranges"):
        assert (bw >= lo[0]).all() and (bw <= hi[0]).all()      # every env has restarted since: its link is of the new ranges
    else:
        assert (bw >= 100.0).all() and (bw <= 500.0).all() and len(np.unique(bw)) > n // 2
    assert np.array_equal(env.state("bw").cpu().numpy(), np.array([o.params()[0] for o in oenvs]))
    # the shadows were in use before the change, and they came back after the last one
    assert swaps["before"] > 0 and swaps["end"] > swaps["at_last_change"], swaps
    env.check_flags()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5. infinite actions
@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("path", ["lists", "noise_sorted"])
def test_infinite_and_overflowing_rate_actions_match_oracle(path, f64):
    """+inf, -inf, +1e308 and -1e308 among U(-1, 1.5) rate actions, as float64 and as float32 (where 1e308 is inf already: the
    oracle is fed the float32 values): +-inf is not NaN, inf * scale is inf, and the clamp absorbs rate * inf and rate / inf in
    both implementations -- no flag.  On the one-sender work-list path (apply_rate_delta) and the one-sender noise path by sorting
    (its own text of it)."""
    n, T, seed = 256, 30, 15
    acts = extreme_rate_actions(seed, n, T)
    if not f64:
        with np.errstate(over="ignore"):
            acts32 = acts.astype(np.float32)
        acts = acts32.astype(np.float64)
        assert np.isinf(acts).sum() >= 18
    kw = dict(latency_noise=1.1) if path == "noise_sorted" else {}
    ref = oracle.run_batch(acts, seed=seed, **kw)
    env = Env(n, device=DEV, seed=seed, record_steps=True, auto_reset=False, **kw)
    if path == "noise_sorted":
        env.set_tuning(noise_sorted=1)
    obs0 = env.reset().cpu().numpy()
    if f64:
        got = run_gpu(env, acts, T)
    else:
        a = torch.as_tensor(acts32, device=DEV)
        assert a.dtype == torch.float32
        rows, obs, dones = [], [], []
        for t in range(T):
            o, r, d, info = env.step(a[:, t])
            rows.append(info["steps"].clone()); obs.append(o.clone()); dones.append(d.clone())
        torch.cuda.synchronize()
        env.check_flags()
        got = (torch.stack(rows, 1).cpu().numpy(), torch.stack(obs, 1).cpu().numpy(), torch.stack(dones, 1).cpu().numpy())
    same_as_oracle(got, ref, obs0, (path, f64))
    rate = got[0][..., 3]
    assert (rate[acts > 1e300] == 1000.0).all() and (rate[acts < -1e300] == 40.0).all()
    env.close()


def test_huge_window_actions_match_oracle_and_infinite_ones_saturate():
    """Window actions of +-1e6 among U(-1, 1.5), one sender with use_cwnd, against per-env oracle objects: cwnd * (1 + 25 000) and
    cwnd / 25 001 truncate to an integer and clamp to [4, 5000] on both sides.
    Not compared with the oracle: +-inf, or anything that takes cwnd * (1 + a * scale) past 2^63.  The C oracle's (long)c is
    undefined there (x86 gives LONG_MIN, which its clamp turns into 4 where the device gives 5000), and the reference's int(inf)
    raises OverflowError: there is no answer to match.  The device saturates -- c >= 5000 is tested on the double, before the
    conversion -- and that is asserted here on its own: +inf gives 5000, -inf gives 4, no flag."""
    n, T, seed = 256, 24, 16
    env = Env(n, device=DEV, seed=seed, record_steps=True, auto_reset=False, use_cwnd=True)
    oenvs = oracle_envs(n, seed, cwnd=True)
    env.reset()
    for o in oenvs:
        o.reset()
    rs = np.random.RandomState(seed)
    acts = rs.uniform(-1, 1.5, (n, T, 2))
    hit = rs.rand(n, T) < 0.08
    acts[..., 1] = np.where(hit, rs.choice([-1e6, 1e6], (n, T)), acts[..., 1])
    osteps = np.zeros(n, dtype=int)
    for t in range(T):
        step_against_oracle_envs(env, oenvs, acts[:, t], osteps, 400, t, cwnd=True)
    env.check_flags()
    a = torch.zeros((n, 2), dtype=torch.float64, device=DEV)
    a[0::2, 1] = float("inf")
    a[1::2, 1] = float("-inf")
    env.step(a)
    cw = env.state("cwnd")[0].cpu().numpy()
    assert (cw[0::2] == 5000).all() and (cw[1::2] == 4).all()
    env.step(torch.zeros((n, 2), dtype=torch.float64, device=DEV))      # (and the windows are sent under)
    env.check_flags()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the refusal
def test_delta_scale_outside_its_domain_is_refused():
    """pcc_set_delta_scale takes a finite value > 0 (include/pcc_sim.h): NaN, +-inf, 0 and a negative value are PCC_EINVAL with a
    message, the handle's value stays (0.2 here, so that "stays" is not "is the default again"), and the constructor raises for
    the same.  By refusal only: no handle with such a value is ever stepped."""
    n, T, seed = 256, 6, 17
    a, twin = (Env(n, device=DEV, seed=seed, record_steps=True, auto_reset=False, delta_scale=0.2) for _ in range(2))
    a.reset(); twin.reset()
    for bad in (float("nan"), float("inf"), float("-inf"), 0.0, -0.025):
        rc = a._L.pcc_set_delta_scale(a._h, ctypes.c_double(bad))
        assert rc == -1, bad      # PCC_EINVAL
        with pytest.raises(pcc_rl_amd.PccError) as e:
            native.check(a._L.pcc_set_delta_scale(a._h, ctypes.c_double(bad)))
        assert e.value.code == -1 and "delta_scale" in str(e.value), str(e.value)
        with pytest.raises(ValueError, match="delta_scale"):
            Env(n, device=DEV, seed=seed, delta_scale=bad)
    acts = actions(seed, n, T)
    got, want = run_gpu(a, acts, T), run_gpu(twin, acts, T)
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    same_as_oracle(got, oracle.run_batch(acts, seed=seed, delta_scale=0.2))
    a.close(); twin.close()
