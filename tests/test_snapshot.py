"""Snapshot and restore of a handle (pcc_snapshot / pcc_restore), on the GPU: a restored handle must go on exactly as the
snapshotted one did.  Every comparison is torch.equal -- observations, rewards, dones, the 19 step columns, every env.state() field,
restart statistics -- against an uninterrupted run of the same library (which the parity suite pins to the oracle).  Actions are
U(-1, 1.5) from a seeded generator, as in the parity file.  With the conftest default the work lists are on at every batch size;
the small-batch tests switch them off themselves."""
import io

import pytest
import torch

import pcc_rl_amd
from pcc_rl_amd import native

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOLS = (2, 8, 32)   # explicit pools: the library's default sizes depend on the free device memory, and two handles must agree


def make_env(n, lists=True, **kw):
    """A BatchedNetworkEnv with the work lists on at every size (lists=True: what the conftest sets for a test) or the library's
    default threshold (the small-batch path below 8192 envs) -- also from a module-scoped fixture, which runs before the conftest's."""
    B = pcc_rl_amd.BatchedNetworkEnv
    old = B.DEFAULT_LIST_MIN_ENVS
    B.DEFAULT_LIST_MIN_ENVS = 0 if lists else None
    try:
        kw.setdefault("ring_pools", POOLS)
        kw.setdefault("record_steps", True)
        return B(n, device=DEV, **kw)
    finally:
        B.DEFAULT_LIST_MIN_ENVS = old


def actions(seed, T, *shape):
    a = torch.rand((T,) + shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2.5 - 1.0
    return a.to(DEV)


def run(env, acts, t0, t1):
    """Steps t0 .. t1-1; every step's (obs, reward, done, step columns), cloned."""
    out = []
    for t in range(t0, t1):
        o, r, d, info = env.step(acts[t])
        out.append((o.clone(), r.clone(), d.clone(), info["steps"].clone()))
    return out


def state_of(env):
    s = {name: env.state(name) for name in native.FIELDS}
    s["restart_stats"] = env.restart_stats()
    return s


def assert_same_steps(a, b):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for k, name in enumerate(("obs", "reward", "done", "steps")):
            assert torch.equal(x[k], y[k]), (t, name)


def assert_same_state(a, b):
    for name in a:
        if name == "restart_stats":
            assert a[name] == b[name], name
        else:
            assert torch.equal(a[name], b[name]), name


def dirty(env, seed=99, steps=5):
    """A fresh handle's rings, lists and blocks filled with OTHER bytes before it is restored over."""
    env.reset()
    a = actions(seed, steps, env.n_envs, *((env.n_senders,) if env.n_senders > 1 else ()), *((2,) if env.use_cwnd else ()))
    for t in range(steps):
        env.step(a[t])


@pytest.fixture(scope="module")
def base():
    """777 envs, max_steps = 30 (an episode boundary between the snapshot and the end), 40 steps with a snapshot after step 12: the
    snapshot, the actions, and what run A returned from there on."""
    n, T, cut = 777, 40, 12
    acts = actions(1, T, n)
    env = make_env(n, seed=5, max_steps=30)
    env.reset()
    head = run(env, acts, 0, cut)
    snap = env.snapshot()
    tail = run(env, acts, cut, T)
    ref = {"n": n, "T": T, "cut": cut, "acts": acts, "snap": snap, "head": head, "tail": tail, "state": state_of(env), "env": env}
    yield ref
    env.close()


def test_same_handle_replay_across_an_episode_boundary(base):
    env, acts = base["env"], base["acts"]
    env.restore(base["snap"])
    assert env._t == base["cut"]
    again = run(env, acts, base["cut"], base["T"])
    assert_same_steps(base["tail"], again)
    assert_same_state(base["state"], state_of(env))
    env.check_flags()
    # taking the snapshot changed nothing: a twin that never took one
    twin = make_env(base["n"], seed=5, max_steps=30)
    twin.reset()
    assert_same_steps(base["head"] + base["tail"], run(twin, acts, 0, base["T"]))
    assert_same_state(base["state"], state_of(twin))
    twin.close()


@pytest.mark.parametrize("through_file", [False, True])
def test_fresh_handle_continues_like_the_original(base, through_file):
    snap = base["snap"]
    if through_file:
        f = io.BytesIO()
        torch.save(snap.to("cpu"), f)
        f.seek(0)
        snap = torch.load(f)
        assert snap.data.device.type == "cpu" and snap.t == base["cut"] and snap.config == base["snap"].config
    env = make_env(base["n"], seed=5, max_steps=30)
    dirty(env)
    env.restore(snap)
    assert_same_steps(base["tail"], run(env, base["acts"], base["cut"], base["T"]))
    assert_same_state(base["state"], state_of(env))
    env.close()


def snapshot_then_fresh(n, cut, more, seed, n_senders=1, **kw):
    """cut steps, snapshot, `more` steps; a fresh (dirtied) handle restored from the snapshot must return the same `more` steps and
    end in the same state."""
    shape = (n, n_senders) if n_senders > 1 else (n,)
    acts = actions(seed, cut + more, *shape)
    env = make_env(n, seed=seed, n_senders=n_senders, **kw)
    env.reset()
    run(env, acts, 0, cut)
    snap = env.snapshot()
    want, want_state = run(env, acts, cut, cut + more), state_of(env)
    env.check_flags()
    other = make_env(n, seed=seed, n_senders=n_senders, **kw)
    dirty(other)
    other.restore(snap)
    assert_same_steps(want, run(other, acts, cut, cut + more))
    assert_same_state(want_state, state_of(other))
    other.close()
    env.close()


def test_ragged_partitions():
    """8 193 envs: eight partitions, the last one of a single env."""
    snapshot_then_fresh(8193, 7, 15, seed=2)


def test_two_senders():
    snapshot_then_fresh(520, 9, 12, seed=4, n_senders=2, history_len=3)


def test_out_of_lockstep_with_shadows():
    """The schedule of test_envs_out_of_lockstep_match_oracle: masked resets at t % 7 == 3, auto-resets at every env's own episode
    end.  The uninterrupted run must start episodes BOTH ways after the snapshot -- by swapping in a shadow and through the restart
    list -- or the test does not reach what it is for.  After t = 40 this schedule starts none through the restart list any more
    (39 by then and 39 at the end; shadow swaps go from 19 to 134): its restart-list starts are the envs that finish before their
    first shadow exists, around t = 29.  So the snapshot is taken after t = 20, when the shadows of the envs masked at t = 3, 10
    and 17 exist and refills are in flight, and both kinds of start follow."""
    n, seed, max_steps, T, cut = 96, 11, 30, 85, 20
    acts = actions(5, T, n)
    idx = torch.arange(n)

    def drive(env, t0, t1):
        out = []
        for t in range(t0, t1):
            if t % 7 == 3:
                out.append(("reset", env.reset((idx % 5) == ((t // 7) % 5)).clone()))
            o, r, d, info = env.step(acts[t])
            out.append((o.clone(), r.clone(), d.clone(), info["steps"].clone()))
        return out

    def same(a, b):
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            if isinstance(x[0], str):
                assert isinstance(y[0], str) and torch.equal(x[1], y[1]), k
            else:
                assert all(torch.equal(p, q) for p, q in zip(x, y)), k

    env = make_env(n, seed=seed, max_steps=max_steps)
    env.reset()
    drive(env, 0, cut + 1)
    snap = env.snapshot()
    at_cut = env.restart_stats()
    want = drive(env, cut + 1, T)
    want_state = state_of(env)
    after = want_state["restart_stats"]
    assert after["shadow_swaps"] > at_cut["shadow_swaps"] and after["restart_list"] > at_cut["restart_list"], (at_cut, after)
    env.check_flags()
    # same handle
    env.restore(snap)
    assert env.restart_stats() == at_cut
    same(want, drive(env, cut + 1, T))
    assert_same_state(want_state, state_of(env))
    env.close()
    # a fresh handle that never left lockstep (it has no shadow rings yet)
    other = make_env(n, seed=seed, max_steps=max_steps)
    dirty(other)
    other.restore(snap)
    same(want, drive(other, cut + 1, T))
    assert_same_state(want_state, state_of(other))
    other.close()


def test_small_batch_path_with_step_many():
    """Below the work-list threshold the steps up to an episode boundary are ONE launch: both sides of the snapshot as step_many."""
    n, cut, more = 777, 12, 28
    acts = actions(7, cut + more, n)
    env = make_env(n, lists=False, seed=8, max_steps=30)
    env.reset()

    def many(e, t0, t1):
        T = t1 - t0
        out = (torch.empty((T, n, 1, e.obs_dim), device=DEV), torch.empty((T, n, 1), device=DEV),
               torch.empty((T, n), dtype=torch.uint8, device=DEV), torch.empty((T, n, 1, native.PCC_STEP_COLS), dtype=torch.float64, device=DEV))
        e.step_many(acts[t0:t1], *out)
        return out

    many(env, 0, cut)
    snap = env.snapshot()
    want, want_state = many(env, cut, cut + more), state_of(env)
    for target in (env, make_env(n, lists=False, seed=8, max_steps=30)):
        if target is not env:
            dirty(target)
        target.restore(snap)
        got = many(target, cut, cut + more)
        assert all(torch.equal(a, b) for a, b in zip(want, got))
        assert_same_state(want_state, state_of(target))
        target.check_flags()
        target.close()


def test_ring_tiers_and_compaction():
    """The inputs of test_ring_tiers_promote_and_come_back_at_reset: upward-drifting actions move senders into the pool tiers.  The
    snapshot holds exactly the live records -- counted here through env.state(), an independent path -- and is smaller than tier 0
    alone."""
    n = 2048
    gen = torch.Generator(device=DEV).manual_seed(0)
    acts = torch.stack([torch.rand(n, generator=gen, device=DEV) * 2 - 0.5 for _ in range(130)])
    env = make_env(n, seed=3, auto_reset=False, ring_pools=(1, 1, 1))
    env.reset()
    run(env, acts, 0, 100)
    assert int(env.state("ring_tier").max().item()) >= 2
    live = int(((env.state("acc_tail") - env.state("acc_head")).long() + (env.state("drop_tail") - env.state("drop_head")).long()).sum().item())
    snap = env.snapshot()
    head = snap.header()
    print("ring tiers: %d live records, snapshot %d bytes (header says %d records), tier 0 alone %d bytes"
          % (live, snap.nbytes, head["ring_records"], n * 3 * 512 * 16))
    assert head["ring_records"] == live and not head["truncated"] and head["total_bytes"] == snap.nbytes
    assert snap.nbytes < n * 3 * 512 * 16
    want, want_state = run(env, acts, 100, 130), state_of(env)
    env.check_flags()
    other = make_env(n, seed=3, auto_reset=False, ring_pools=(1, 1, 1))
    dirty(other)
    other.restore(snap)
    assert_same_steps(want, run(other, acts, 100, 130))
    assert_same_state(want_state, state_of(other))
    other.check_flags()
    other.close()
    env.close()


def test_trace_rng_same_handle():
    n, cut, more = 64, 8, 10
    u = torch.rand((n, 60000), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    acts = actions(9, cut + more, n)
    env = make_env(n, seed=1, max_steps=400)
    env.set_loss_trace(u)
    env.reset()
    run(env, acts, 0, cut)
    snap = env.snapshot()
    want, want_state = run(env, acts, cut, cut + more), state_of(env)
    env.check_flags()
    env.restore(snap)
    assert_same_steps(want, run(env, acts, cut, cut + more))
    assert_same_state(want_state, state_of(env))
    env.close()


def test_use_cwnd_one_sender_same_handle():
    n, cut, more = 256, 8, 10
    acts = actions(10, cut + more, n, 2)
    env = make_env(n, seed=6, use_cwnd=True)
    env.reset()
    run(env, acts, 0, cut)
    snap = env.snapshot()
    want, want_state = run(env, acts, cut, cut + more), state_of(env)
    env.restore(snap)
    assert_same_steps(want, run(env, acts, cut, cut + more))
    assert_same_state(want_state, state_of(env))
    env.close()


def test_closed_loop_rollout():
    """1 024 envs on the small-batch path, the policy inside the step launches (env.rollout, deterministic)."""
    from pcc_rl_amd.ppo import MlpPolicy
    n, T = 1024, 8
    env = make_env(n, lists=False, seed=12, record_steps=False)
    torch.manual_seed(0)
    params = MlpPolicy(env.obs_dim, 1, (32, 16)).to(DEV).flat_params()

    def roll(obs0):
        bufs = (torch.empty((T + 1, n, env.obs_dim), device=DEV), torch.empty((T, n, 1), device=DEV), torch.empty((T, n), device=DEV),
                torch.empty((T, n), device=DEV), torch.empty((T, n), device=DEV), torch.empty((T, n), dtype=torch.uint8, device=DEV))
        bufs[0][0] = obs0
        env.rollout(params, None, *bufs)
        return bufs

    first = roll(env.reset())
    snap = env.snapshot()
    want, want_state = roll(first[0][T]), state_of(env)
    env.restore(snap)
    got = roll(first[0][T])
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    assert_same_state(want_state, state_of(env))
    env.close()


def test_refusals_leave_the_target_untouched():
    """Host-side validation only (no buffer's payload is ever tampered with): what is refused, with which code, and that a refused
    restore has not touched its target -- its next steps equal its own twin's."""
    n = 1024   # (pools of n / 2 and n / 4 slots differ; below 256 slots every pool has 256)
    acts = actions(13, 12, n)
    src = make_env(n, seed=21)
    src.reset()
    run(src, acts, 0, 4)
    snap = src.snapshot()
    # the event-loop build is not snapshotted
    noisy = make_env(64, seed=1, latency_noise=1.1)
    noisy.reset()
    with pytest.raises(pcc_rl_amd.PccError) as e:
        noisy.snapshot()
    assert e.value.code == -1 and "event-loop" in str(e.value)
    noisy.close()
    # ... nor a handle with the one-launch step on (its ready queues)
    fused = make_env(512, seed=1)
    fused.reset()
    fused.set_tuning(fused=1)
    with pytest.raises(pcc_rl_amd.PccError) as e:
        fused.snapshot()
    assert e.value.code == -1 and "PCC_TUNE_FUSED" in str(e.value)
    with pytest.raises(pcc_rl_amd.PccError) as e:
        native.check(native.lib().pcc_restore(fused._h, pcc_rl_amd.env._ptr(snap.data), snap.nbytes, fused._stream()))
    assert e.value.code == -1 and "PCC_TUNE_FUSED" in str(e.value)
    fused.close()
    # between the two halves of a step
    src.step_send(acts[4])
    with pytest.raises(pcc_rl_amd.PccError) as e:
        src.snapshot()
    assert e.value.code == -5
    with pytest.raises(pcc_rl_amd.PccError) as e:
        src.restore(snap)
    assert e.value.code == -5
    src.step_retire()
    src.restore(snap)   # (back to where the snapshot was taken: the comparison at the end starts there)

    def refused(target, twin, how, code=-1, names=None, width=None):
        """`how(target)` must raise; then target and twin, stepped alike, agree (width: components per action, with use_cwnd 2)."""
        with pytest.raises((pcc_rl_amd.PccError, ValueError)) as e:
            how(target)
        if isinstance(e.value, pcc_rl_amd.PccError):
            assert e.value.code == code
        if names:
            assert names in str(e.value), str(e.value)
        m = target.n_envs
        a = actions(14, 3, m, *((width,) if width else ()))
        assert_same_steps(run(target, a, 0, 3), run(twin, a, 0, 3))
        assert_same_state(state_of(target), state_of(twin))

    def pair(m, **kw):
        a, b = make_env(m, **kw), make_env(m, **kw)
        dirty(a, seed=15, steps=2)
        dirty(b, seed=15, steps=2)
        return a, b

    L = native.lib()

    def raw_restore(env, data=None, nbytes=None):
        data = snap.data if data is None else data
        native.check(L.pcc_restore(env._h, pcc_rl_amd.env._ptr(data), int(data.numel() if nbytes is None else nbytes), env._stream()))

    # through the Python checks (readable messages) ...
    for kw, field in (({"seed": 22}, "seed"), ({"seed": 21, "ring_pools": (4, 8, 32)}, "ring_pools")):
        a, b = pair(n, **kw)
        refused(a, b, lambda e: e.restore(snap), names=field)
        a.close(); b.close()
    a, b = pair(n + 1, seed=21)
    refused(a, b, lambda e: e.restore(snap), names="n_envs")
    # ... and straight through the C ABI: PCC_EINVAL, the message names the field
    refused(a, b, raw_restore, names="envs")
    a.close(); b.close()
    a, b = pair(n, seed=22)
    refused(a, b, raw_restore, names="seed")
    a.close(); b.close()
    a, b = pair(n, seed=21, ring_pools=(4, 8, 32))
    refused(a, b, raw_restore, names="ring pool slots")
    a.close(); b.close()
    # the rest of the configuration the header names (include/pcc_sim.h), one field at a time, straight through the C ABI: a
    # target that differs from the source in the delta scale, one bound of the parameter ranges, max steps, or in having link
    # arrays where the source has none
    slow = ((20.0, 0.01, 0.0, 0.3, 0.1), (60.0, 0.02, 1.0, 0.9, 4.0))
    default_but_one = ((100.0, 0.05, 0.0, 0.0, 0.3), (500.0, 0.5, 8.0, 0.0625, 1.5))   # (the loss range's upper bound: 0.05 -> 0.0625)
    for kw, setup, field in (({"delta_scale": 0.2}, None, "delta scale"),
                             ({}, lambda e: e.randomize_link_params(default_but_one), "parameter ranges"),
                             ({"max_steps": 399}, None, "max steps"),
                             ({}, lambda e: e.set_link_params(200.0, 0.03, 5.0, 0.0, 60.0), "link parameter arrays")):
        a, b = make_env(n, seed=21, **kw), make_env(n, seed=21, **kw)
        for e in (a, b):
            if setup:
                setup(e)
            dirty(e, seed=15, steps=2)
        refused(a, b, raw_restore, names=field)
        a.close(); b.close()
    # ... and the cwnd mode, on one-sender handles both ways (a window-limited target and a plain snapshot, and the reverse)
    a, b = pair(n, seed=21, use_cwnd=True)
    refused(a, b, raw_restore, names="cwnd mode", width=2)
    cw_snap = a.snapshot()
    a.close(); b.close()
    a, b = pair(n, seed=21)
    refused(a, b, lambda e: raw_restore(e, data=cw_snap.data), names="cwnd mode")
    a.close(); b.close()
    a, b = pair(n, seed=21)
    refused(a, b, lambda e: raw_restore(e, nbytes=snap.nbytes - 16), names="bytes")
    refused(a, b, lambda e: raw_restore(e, nbytes=64), names="bytes")
    refused(a, b, lambda e: raw_restore(e, data=torch.zeros(snap.nbytes, dtype=torch.uint8, device=DEV)), names="magic")
    # and the same target still takes the snapshot
    a.restore(snap)
    assert_same_steps(run(a, acts, 4, 12), run(src, acts, 4, 12))
    a.close(); b.close()
    src.close()


def test_settings_off_their_defaults_are_carried_out_of_lockstep():
    """The positive side of the configuration check: delta_scale = 0.2 and sampling ranges of slow, lossy, shallow links (bw 20-60,
    up to nine packets in ten lost, starting rates below MIN_RATE), masked resets that take the envs out of lockstep, a snapshot
    with shadows prepared from those ranges; a fresh handle of the same settings continues bit for bit over every env's next
    episode boundary (episodes of 20 steps, 30 more steps), and ends in the same state."""
    n, seed, max_steps, cut, T = 96, 23, 20, 24, 54
    slow = ((20.0, 0.01, 0.0, 0.3, 0.1), (60.0, 0.02, 1.0, 0.9, 4.0))
    acts = actions(19, T, n)
    idx = torch.arange(n)

    def make():
        env = make_env(n, seed=seed, max_steps=max_steps, delta_scale=0.2)
        env.randomize_link_params(slow)
        return env

    def drive(env, t0, t1):
        out = []
        for t in range(t0, t1):
            if t < 20 and t % 5 == 2:
                out.append(env.reset((idx % 4) == ((t // 5) % 4)).clone())
            o, r, d, info = env.step(acts[t])
            out += [o.clone(), r.clone(), d.clone(), info["steps"].clone()]
        return out

    env = make()
    env.reset()
    drive(env, 0, cut)
    snap = env.snapshot()
    assert snap.config["delta_scale"] == 0.2
    want, want_state = drive(env, cut, T), state_of(env)
    bw = want_state["bw"]
    assert bool(((bw >= 20.0) & (bw <= 60.0)).all()) and want_state["restart_stats"]["shadow_swaps"] > 0
    assert bool(torch.stack(want[2::4]).any(0).all())   # (no masked reset after the cut: four entries a step; every env ended an episode)
    env.check_flags()
    other = make()
    dirty(other)
    other.restore(snap)
    got = drive(other, cut, T)
    assert len(got) == len(want) and all(torch.equal(x, y) for x, y in zip(want, got))
    assert_same_state(want_state, state_of(other))
    other.check_flags()
    other.close()
    env.close()


@pytest.mark.parametrize("src_lists", [True, False])
def test_work_lists_are_a_knob_not_configuration(src_lists):
    """list_min_envs is a performance knob: a snapshot taken from a handle that steps with work lists restores into one that steps
    without them (the small-batch path), and the other way round, and the continuation is the original's."""
    n, cut, more = 777, 9, 25
    acts = actions(17, cut + more, n)
    env = make_env(n, lists=src_lists, seed=14, max_steps=30)
    env.reset()
    run(env, acts, 0, cut)
    snap = env.snapshot()
    want, want_state = run(env, acts, cut, cut + more), state_of(env)
    other = make_env(n, lists=not src_lists, seed=14, max_steps=30)
    dirty(other)
    other.restore(snap)
    assert_same_steps(want, run(other, acts, cut, cut + more))
    assert_same_state(want_state, state_of(other))
    other.check_flags()
    other.close()
    env.close()


def test_simulated_env_passes_through():
    """SimulatedNetworkEnv (the reference's single-env protocol): the snapshot carries the adapter's own float64 history and
    counters next to the simulator's state, also through to("cpu") and a file."""
    import numpy as np
    a = torch.rand(20, generator=torch.Generator().manual_seed(18), dtype=torch.float64).numpy() * 2.5 - 1.0
    env = pcc_rl_amd.SimulatedNetworkEnv(device=DEV, seed=3)
    env.reset()
    for t in range(6):
        env.step([a[t]])
    snap = env.snapshot()
    want = [env.step([a[t]]) for t in range(6, 14)]
    f = io.BytesIO()
    torch.save(snap.to("cpu"), f)
    f.seek(0)
    other = pcc_rl_amd.SimulatedNetworkEnv(device=DEV, seed=3)
    other.reset()
    for t in range(3):
        other.step([a[19 - t]])
    other.restore(torch.load(f))
    assert other.steps_taken == 6
    got = [other.step([a[t]]) for t in range(6, 14)]
    for (o1, r1, d1, _), (o2, r2, d2, _) in zip(want, got):
        assert o1.dtype == np.float64 and np.array_equal(o1, o2) and r1 == r2 and d1 == d2
    assert (other.steps_taken, other.reward_sum, other.run_dur) == (env.steps_taken, env.reward_sum, env.run_dur)
    assert other.event_record == env.event_record
    with pytest.raises(ValueError):
        other.restore(other._env.snapshot())   # (a BatchedNetworkEnv's snapshot holds no adapter state)
    env.close(); other.close()


def test_grouped_env_group_by_group():
    """GroupedNetworkEnv: every group's snapshot and restore on the group's own stream."""
    n, G, cut, more = 512, 2, 6, 8
    acts = actions(16, cut + more, n)
    env = pcc_rl_amd.GroupedNetworkEnv(n, n_groups=G, device=DEV, seed=9, ring_pools=POOLS, record_steps=True)

    def drive(t0, t1):
        out = []
        for t in range(t0, t1):
            for g in range(G):
                o, r, d, info = env.step_group(g, acts[t, g * env.group_size:(g + 1) * env.group_size])
                with torch.cuda.stream(env.streams[g]):   # (the group's output buffers are valid on the group's stream)
                    out.append((o.clone(), r.clone(), d.clone(), info["steps"].clone()))
        env.synchronize()
        return out

    env.reset()
    drive(0, cut)
    snap = env.snapshot()
    want = drive(cut, cut + more)
    env.restore(snap.to("cpu").to(DEV))
    assert_same_steps(want, drive(cut, cut + more))
    env.check_flags()
    env.close()


@pytest.mark.parametrize("policy_in_step", [False, True])
def test_ppo_resumes_bit_for_bit(policy_in_step):
    """2 iterations, state_dict(), 2 more (P_A); a new env and a new PPO load it and do 2 iterations (P_B): the same parameters, the
    same Adam moments, the same reported rewards."""
    from pcc_rl_amd.ppo import PPO

    def fresh():
        env = make_env(1024, lists=False, seed=30, record_steps=False)
        return env, PPO(env, horizon=16, seed=3, policy_in_step=policy_in_step)

    env_a, a = fresh()
    assert a.fused_update
    for _ in range(2):
        a.iterate()
    f = io.BytesIO()
    torch.save(a.state_dict(), f)
    rewards_a = [a.iterate()["mean_step_reward"] for _ in range(2)]
    env_b, b = fresh()
    torch.manual_seed(12345)   # (whatever the process did to the generators in between)
    torch.randn(7, device=DEV)
    f.seek(0)
    b.load_state_dict(torch.load(f))
    rewards_b = [b.iterate()["mean_step_reward"] for _ in range(2)]
    assert rewards_a == rewards_b
    assert torch.equal(a.flat, b.flat) and torch.equal(a.adam_m, b.adam_m) and torch.equal(a.adam_v, b.adam_v) and a.adam_t == b.adam_t
    assert torch.equal(a.obs, b.obs)
    env_a.close(); env_b.close()
