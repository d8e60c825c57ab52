"""The product's own copies of rtt_means at the list lengths the ordinary parity tests rarely or never produce, against the C oracle.

tests/test_rtt_means.py holds the routine to numpy through a harness -- a separate compilation.  rtt_means is compiled into six
product kernels separately (retire_kernel at 8 and at 16 lanes per env, its NOISE build, retire_kernel<1, false, PolicyArgs>,
step_small_kernel / step_small_policy_kernel, step_fused_kernel), and the default link ranges never take any of them past about
7 700 samples: the 8192-sample chunks, and the seventh level of the walk's stack (a chunk of 7 689 .. 8 191 samples), are all but unreachable there.
Three link families do it (tests/test_rtt_means_cpu.py defines them and proves, from the oracle alone, which lengths they reach):
  D  48 deep queues (16 500 .. 19 000 packets) sent into at the maximum rate: every env has lists past 8 192 acknowledgements (a
     full chunk and a remainder: six levels deep), the batch lists on both sides of 8 192 + 128;
  E  the same with queues of 15 350 .. 16 150: every env has at least three lists (915 in all) of 7 689 .. 8 191 samples whose
     tree is seven levels deep -- the only lengths at which the seventh level of the walk's stack is used at all;
  S  512 short links: every length 0 .. 272 at least three times, and lengths up to 2 048.
Every route below is compared bit for bit with oracle.run_batch -- the 19 step columns and the observations, flags clean -- and
the lengths it reached are asserted from the ORACLE's `acked` column: the device is never asked.  PCC_RTT_RECORD=<file> appends
each route's histogram of lengths there (profiles/r22_rtt_lengths.json was made that way)."""
import json
import os

import numpy as np
import pytest
import torch

import oracle
import pcc_rl_amd
from pcc_rl_amd import native
from test_gpu_parity import DEV
from test_rollout import _buffers, _params
from test_rtt_means_cpu import (NOISE_ENVS, NOISE_STEPS, assert_deep_lengths, assert_noise_lengths, assert_seventh_level, assert_short_lengths,
                                assert_two_sender_lengths, family_d, family_e, family_s, fits_the_rings, histogram, lengths_of)

pytestmark = pytest.mark.gpu
Env = pcc_rl_amd.BatchedNetworkEnv
TWO_FEATURES = ("send ratio", "latency ratio")      # neither needs the halves: need_halves == false when no step record is written
LANES = {"8_lanes": dict(retire_wide_predict=1e9), "16_lanes": dict(retire_wide_predict=0.0, retire_grid_frac=1.0)}


def _record(route, family, lengths):
    out = os.environ.get("PCC_RTT_RECORD")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps({"route": route, "family": family, "longest": int(np.max(lengths)), "lengths": histogram(lengths)}, sort_keys=True) + "\n")


def make_env(c, n_senders=1, deep=False, **kw):
    """a handle on the family's links; family D: the default ring_capacity and a slot in every tier of the ring pools for every sender"""
    p = np.array(c["links"])      # (a copy: the family's arrays are read-only)
    kw.setdefault("record_steps", True)
    env = Env(p.shape[0], device=DEV, seed=c["seed"], n_senders=n_senders, auto_reset=False, ring_pools=(1, 1, 1) if deep else None, **kw)
    env.set_link_params(p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4] if n_senders == 1 else p[:, 4:6])
    return env


def same(got, ref, obs0, what, fits=None):
    """every step column and observation bit-equal to the oracle's for the envs that fit their rings (family D; None: all)"""
    steps, obs, done = got
    ok = np.ones(steps.shape[0], dtype=bool) if fits is None else fits
    assert np.array_equal(obs0.reshape(ref["obs0"].shape)[ok], ref["obs0"].astype(np.float32)[ok]), what
    diff = (steps != ref["steps"]).any(axis=-1)                    # [envs, (senders,) steps]
    diff[~ok] = False
    if diff.any():
        lens = sorted({int(v) for v in ref["steps"][..., 1][diff]})
        raise AssertionError("%s: %d rows of %d envs differ from the oracle (first env %d); the lists of those rows: %s"
                             % (what, diff.sum(), diff.reshape(diff.shape[0], -1).any(axis=1).sum(), np.argwhere(diff)[0][0], lens[:40]))
    assert np.array_equal(obs.reshape(ref["obs"].shape)[ok], ref["obs"].astype(np.float32)[ok]), what
    assert not done.any(), what


def flags_clean(env, fits=None):
    flags = env.state("flags").cpu().numpy().astype(np.int64)
    if fits is None:
        env.check_flags()
    assert not flags[np.ones(flags.shape, dtype=bool) if fits is None else fits].any(), np.unique(flags)


def by_steps(env, c, what, fits=None):
    obs0 = env.reset().cpu().numpy()
    acts = torch.as_tensor(np.array(c["acts"]), dtype=torch.float64, device=DEV)      # (a copy: the family's arrays are read-only)
    rows, obs, dones = [], [], []
    for t in range(c["acts"].shape[1]):
        o, _, d, info = env.step(acts[:, t])
        rows.append(info["steps"].clone()); obs.append(o.clone()); dones.append(d.clone())
    torch.cuda.synchronize()
    flags_clean(env, fits)
    ax = 1 if env.n_senders == 1 else 2
    same((torch.stack(rows, ax).cpu().numpy(), torch.stack(obs, ax).cpu().numpy(), torch.stack(dones, 1).cpu().numpy()), c, obs0, what, fits)


def by_step_many(env, c, what, fits=None):
    n, T, S = c["acts"].shape[0], c["acts"].shape[1], env.n_senders
    obs0 = env.reset().cpu().numpy()
    a = torch.as_tensor(np.ascontiguousarray(np.moveaxis(c["acts"], 1, 0)), dtype=torch.float64, device=DEV)
    obs = torch.empty((T, n, S, env.obs_dim), device=DEV)
    rew = torch.empty((T, n, S), device=DEV)
    done = torch.empty((T, n), dtype=torch.uint8, device=DEV)
    rows = torch.empty((T, n, S, native.PCC_STEP_COLS), dtype=torch.float64, device=DEV)
    env.step_many(a, obs, rew, done, rows)
    torch.cuda.synchronize()
    flags_clean(env, fits)
    if S == 1:
        got = (rows[:, :, 0].transpose(0, 1).cpu().numpy(), obs[:, :, 0].transpose(0, 1).cpu().numpy(), done.t().cpu().numpy() != 0)
    else:
        got = (rows.permute(1, 2, 0, 3).cpu().numpy(), obs.permute(1, 2, 0, 3).cpu().numpy(), done.t().cpu().numpy() != 0)
    same(got, c, obs0, what, fits)


DEEP = {"D": (family_d, assert_deep_lengths), "E": (family_e, assert_seventh_level)}


def family(name, features=None):
    """-> (the family's dictionary, its lengths as its own condition returns them -- asserted -- and which envs fit their rings)"""
    kw = {} if features is None else {"features": features}
    if name == "S":
        c = family_s(**kw)
        return c, assert_short_lengths(c, name), None
    c = DEEP[name][0](**kw)
    return c, DEEP[name][1](c, c["fits"], name), c["fits"]


# ------------------------------------------------------------------------------------------------ retire_kernel, 8 and 16 lanes
@pytest.mark.parametrize("lanes", sorted(LANES))
@pytest.mark.parametrize("name", ["D", "E", "S"])
def test_retire_kernel(name, lanes):
    """Through the work lists, by 8 lanes (three walks one after the other) and by 16 (whole list and halves side by side): lists
    past the chunk edge (D), lists that fill the seventh level of the walk's stack in every env (E), every short length (S)."""
    c, n, fits = family(name)
    env = make_env(c, deep=fits is not None)
    env.set_tuning(list_min_envs=0, **LANES[lanes])
    by_steps(env, c, (name, lanes), fits)
    env.close()
    _record("retire_kernel, " + lanes, name, n)


# ------------------------------------------------------------------------------------------------ step_small_kernel
@pytest.mark.parametrize("name", ["D", "E", "S"])
def test_small_batch_kernel(name):
    """pcc_step_many below the work-list threshold: the whole episode inside step_small_kernel's loop."""
    Env.DEFAULT_LIST_MIN_ENVS = None          # (the conftest's fixture puts its 0 back)
    c, n, fits = family(name)
    env = make_env(c, deep=fits is not None)
    by_step_many(env, c, name, fits)
    env.close()
    _record("step_small_kernel", name, n)


# ------------------------------------------------------------------------------------------------ the policy kernels
def by_rollout(c, deep=False):
    """T closed-loop steps; then the oracle fed the actions the rollout took -> (env, got, ref, obs0)"""
    T = c["acts"].shape[1]
    env = make_env(c, deep=deep, record_steps=False)
    env.set_tuning(rollout_epilogue=1)
    env.reset()
    b = _buffers(env, T)
    b["obs"][0].copy_(env._obs)
    noise = torch.randn((T, env.n_envs), device=DEV, generator=torch.Generator(device=DEV).manual_seed(c["seed"]))
    env.rollout(_params(env.obs_dim), noise, b["obs"], b["act"], None, None, None, b["done"], b["steps"])
    torch.cuda.synchronize()
    acts = b["act"][:, :, 0].t().double().cpu().numpy()
    ref = oracle.run_batch(acts, seed=c["seed"], params=c["links"], n_threads=8)
    got = (b["steps"][:, :, 0].transpose(0, 1).cpu().numpy(), b["obs"][1:, :, 0].transpose(0, 1).cpu().numpy(), b["done"].t().cpu().numpy() != 0)
    return env, got, ref, b["obs"][0, :, 0].cpu().numpy()


def rollout_against_the_oracle(name, route):
    """The actions are the policy's, so the family's condition is asserted on the oracle's run of THOSE actions, and so is which
    envs fit their rings.  On the deep families a Gaussian head of log_std -0.7 moves the rates by a few percent a step: they
    stay above every bandwidth (asserted), the queues stay full, and a full queue's lists do not depend on the rate."""
    c = family_s() if name == "S" else DEEP[name][0]()
    env, got, ref, obs0 = by_rollout(c, deep=name != "S")
    n = lengths_of(ref, 1)
    print("%s on family %s, the policy's actions: longest list %d; %s" % (route, name, n.max(), histogram(n)))
    if name == "S":
        n, fits = assert_short_lengths(ref, route), None
    else:
        assert (ref["steps"][..., 3] > c["links"][:, 0:1]).all()       # every rate above its link's bandwidth, every step
        fits = fits_the_rings(ref, c["links"])
        n = DEEP[name][1](ref, fits, route)
    flags_clean(env, fits)
    same(got, ref, obs0, (route, name), fits)
    env.close()
    _record(route, name, n)


@pytest.mark.parametrize("name", ["D", "E", "S"])
def test_retire_kernel_with_the_policy_epilogue(name):
    """rollout_epilogue = 1 on the list path: retire_kernel<1, false, PolicyArgs>."""
    rollout_against_the_oracle(name, "retire_kernel<1, false, PolicyArgs>")


def test_small_batch_policy_kernel():
    """the same below the work-list threshold: step_small_policy_kernel"""
    Env.DEFAULT_LIST_MIN_ENVS = None
    rollout_against_the_oracle("S", "step_small_policy_kernel")


# ------------------------------------------------------------------------------------------------ two senders
@pytest.mark.parametrize("path", ["lists", "small_batch"])
def test_two_senders(path):
    """Two senders on one bottleneck: two lists per env, of different lengths, one after the other in the same group."""
    if path == "small_batch":
        Env.DEFAULT_LIST_MIN_ENVS = None
    c = family_s(n_senders=2)
    n = assert_two_sender_lengths(c)
    env = make_env(c, n_senders=2)
    (by_steps if path == "lists" else by_step_many)(env, c, path)
    env.close()
    _record("two senders, " + path, "S", n)


# ------------------------------------------------------------------------------------------------ latency noise
@pytest.mark.parametrize("noise_sorted", [0, 1])
def test_latency_noise_builds(noise_sorted):
    """latency_noise = 1.1: the samples are whole RTTs and dl == 0.0 in the call.  noise_sorted = 0: the event loop for every env
    (retire_kernel's NOISE build); 1: the sorting kernels, which leave the RTTs in noise_rtt for the same routine."""
    c = family_s(latency_noise=1.1, n=NOISE_ENVS, steps=NOISE_STEPS)
    n = assert_noise_lengths(c)
    env = make_env(c, latency_noise=1.1)
    env.set_tuning(noise_sorted=noise_sorted)
    by_steps(env, c, noise_sorted)
    env.close()
    _record("latency noise, noise_sorted=%d" % noise_sorted, "S", n)


# ------------------------------------------------------------------------------------------------ the one-launch step
def test_one_launch_step():
    c = family_s()
    n = assert_short_lengths(c)
    env = make_env(c)
    env.set_tuning(list_min_envs=0, fused=1)
    by_steps(env, c, "fused")
    assert env.fused_steps() == c["acts"].shape[1] - 1, env.fused_steps()       # (the step after the reset has no lists yet)
    env.close()
    _record("step_fused_kernel", "S", n)


# ------------------------------------------------------------------------------------------------ need_halves == false
@pytest.mark.parametrize("lanes", sorted(LANES))
@pytest.mark.parametrize("name", ["D", "E", "S"])
def test_without_the_halves(name, lanes):
    """Features that need no latency increase, stepped with env.step and no step record: rtt_means is called with need_halves ==
    false (one walk, no pairing).  The oracle runs with the same features; observations and rewards are compared -- float32, which a
    1-ulp difference of a mean only reaches when it flips a packet count, and on a full queue it never does -- and, in float64, the
    state fields the mean goes into: run_dur (half the mean) and the clock."""
    c, n, fits = family(name, TWO_FEATURES)
    deep = fits is not None
    fits = fits if deep else np.ones(c["acts"].shape[0], dtype=bool)
    env = make_env(c, deep=deep, features=list(TWO_FEATURES), record_steps=False)
    env.set_tuning(list_min_envs=0, **LANES[lanes])
    obs0 = env.reset().cpu().numpy()
    assert np.array_equal(obs0[fits], c["obs0"].astype(np.float32)[fits])
    acts = torch.as_tensor(np.array(c["acts"]), dtype=torch.float64, device=DEV)      # (a copy: the family's arrays are read-only)
    obs, rew, now, dur = [], [], [], []
    for t in range(c["acts"].shape[1]):
        o, r, d, info = env.step(acts[:, t])
        assert "steps" not in info
        obs.append(o.clone()); rew.append(r.clone()); now.append(env.state("now")); dur.append(env.state("run_dur"))
    torch.cuda.synchronize()
    flags_clean(env, fits if deep else None)
    obs, rew = torch.stack(obs, 1).cpu().numpy(), torch.stack(rew, 1).cpu().numpy()
    # the mean itself in float64: the next interval's length is half of it, and the clock adds them up
    assert np.array_equal(torch.stack(dur, 1).cpu().numpy()[fits], c["steps"][..., 5][fits]), (name, lanes)
    assert np.array_equal(torch.stack(now, 1).cpu().numpy()[fits], c["steps"][..., 4][fits]), (name, lanes)
    assert np.array_equal(obs[fits], c["obs"].astype(np.float32)[fits]), (name, lanes)
    assert np.array_equal(rew[fits], c["steps"][..., 6].astype(np.float32)[fits]), (name, lanes)
    env.close()
    _record("need_halves == false, " + lanes, name, n)
