"""Reward normalisation, the part that needs no GPU (include/pcc_policy.h: pcc_return_stats_update_pop, pcc_reward_normalise_pop
and their stand-alone forms): the numpy restatement of tests/models/reward_norm_model.py held against
itself (the split-call identity, the kernels' own order of the sums against the float64 two-pass), the five symbols, every refusal
of the host side, the compiler's resource report of the three kernels, and what the constructors refuse."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import reward_norm_model as model  # noqa: E402

from pcc_rl_amd import native  # noqa: E402
from pcc_rl_amd.native import lib  # noqa: E402
from pcc_rl_amd.ppo import PPO, PopulationPPO  # noqa: E402
from pcc_rl_amd.rewnorm import RewardNormalizer  # noqa: E402

RET_SYMBOLS = {"pcc_return_scratch_doubles": 3, "pcc_return_stats_update_pop": 13, "pcc_reward_normalise_pop": 8,
               "pcc_return_stats_update": 11, "pcc_reward_normalise": 7}
# (T, n_m): the edges of the wavefront and the workgroup, several workgroups, more workgroups than the merge has sub-lanes (a
# sub-lane then sums two partials), and a whole episode's length
MODEL_SHAPES = ((1, 1), (5, 257), (7, 4099), (3, 65), (3, 64), (400, 64), (2, 256 * 300 + 1))
GAMMAS = (0.99, 0.0, 1.0)


# ---------------------------------------------------------------------------------------------------------- the model alone
@pytest.mark.parametrize("kind", model.REWARD_KINDS)
def test_split_calls_leave_the_same_carry(kind):
    """[0, T) in one call and in two: the same ret_carry bits and count; the other moments within the bound."""
    rng = np.random.default_rng(11)
    for T, N, K, T1 in ((9, 12, 3, 4), (400, 6, 2, 1), (2, 64, 1, 1)):
        r, d = model.make_rewards(kind, (T, N), rng), model.make_done("bernoulli", (T, N), rng)
        gammas = np.array([0.99, 0.9, 1.0], dtype=np.float32)[:K]
        start = rng.standard_normal(N) * 10.0
        whole, carry = model.walk(r, d, gammas, start)
        first, mid = model.walk(r[:T1], d[:T1], gammas, start)
        second, end = model.walk(r[T1:], d[T1:], gammas, mid)
        assert np.array_equal(carry.view(np.int64), end.view(np.int64))
        assert np.array_equal(np.concatenate([first, second]).view(np.int64), whole.view(np.int64))
        empty = np.zeros((K, 3))
        one = model.update_stats(empty, whole, K)
        two = model.update_stats(model.update_stats(empty, first, K), second, K)
        for m in range(K):
            b_mean, b_var = model.moment_bounds(one[m, 0], float(np.abs(model.member_samples(whole, m, K)).max()))
            assert one[m, 0] == two[m, 0] == T * N // K
            assert abs(one[m, 1] - two[m, 1]) <= b_mean and abs(one[m, 2] - two[m, 2]) / one[m, 0] <= b_var, (T, N, m)


def test_the_walk_takes_the_sample_before_the_reset():
    r = np.array([[1.0], [2.0], [4.0], [8.0]], dtype=np.float32)
    d = np.array([[0], [1], [0], [0]], dtype=np.uint8)
    samples, carry = model.walk(r, d, [0.5], [16.0])
    assert samples[:, 0].tolist() == [9.0, 6.5, 4.0, 10.0] and carry.tolist() == [10.0]
    g = np.float32(0.99)
    samples, _ = model.walk(np.full((2, 1), 0.1, np.float32), np.zeros((2, 1), np.uint8), [0.99], [0.0])
    r0 = np.float64(np.float32(0.1))
    assert samples[1, 0] == r0 * np.float64(g) + r0                       # (the float32 gamma, widened: not 0.99)
    assert model.scale_from_stats(np.array([[4.0, 1.5, 16.0, 99.0]]), 0.0).tolist() == [0.5]
    out = model.normalise(np.array([[3.0, -3.0, 1e30, np.nan]], dtype=np.float32), np.array([2.0, 1e30], dtype=np.float32), 2, 5.0)
    assert out.tolist() == [[5.0, -5.0, 5.0, -5.0]]                       # (fmax(NaN, -clip) = -clip, like fmaxf)


@pytest.mark.parametrize("kind", model.REWARD_KINDS)
def test_the_kernels_order_of_the_sums_is_within_the_bound(kind):
    """lane over T, a tree over the workgroup, the partials in index order -- against the float64 two-pass, and how much of
    moment_bounds it uses at the most."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for T, n_m in MODEL_SHAPES:
        for gamma in GAMMAS:
            for done_kind in model.DONE_KINDS:
                r, d = model.make_rewards(kind, (T, n_m), rng), model.make_done(done_kind, (T, n_m), rng)
                samples, _ = model.walk(r, d, [gamma], np.zeros(n_m))
                n, mean, m2 = model.batch_moments(samples.reshape(-1, 1))
                gn, gmean, gm2 = model.kernel_order_moments(samples)
                b_mean, b_var = model.moment_bounds(n, float(np.abs(samples).max()))
                assert gn == n == T * n_m
                e_mean, e_var = abs(gmean - mean[0]), abs(gm2 - m2[0]) / n
                assert e_mean <= b_mean and e_var <= b_var and gm2 >= 0.0, (T, n_m, gamma, done_kind, e_mean, b_mean, e_var, b_var)
                worst = max(worst, e_mean / b_mean if b_mean else 0.0, e_var / b_var if b_var else 0.0)
    print("the kernels' order uses at most %.4f %% of the bound (%s)" % (100.0 * worst, kind))


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_five_symbols_are_exported():
    L = lib()
    for s, n_args in RET_SYMBOLS.items():
        assert s in native.SYMBOLS, s
        assert hasattr(L, s), s
        assert len(getattr(L, s).argtypes) == n_args, s


def test_scratch_size():
    L = lib()
    for T, N, K, want in ((1, 1, 1, 3), (5, 771, 3, 3 * 2 * 3), (64, 65536, 8, 8 * 32 * 3), (64, 65536, 1, 256 * 3), (400, 64, 1, 3),
                          (1, 1024, 1024, 1024 * 3), (3, 256, 1, 3), (3, 257, 1, 6)):
        assert L.pcc_return_scratch_doubles(T, N, K) == want, (T, N, K)
    for T, N, K in ((0, 8, 1), (-1, 8, 1), (4, 8, 0), (4, 2050, 1025), (4, 9, 2), (4, 0, 1), (4, -8, 1)):
        assert L.pcc_return_scratch_doubles(T, N, K) == -1, (T, N, K)


def test_refusals_need_no_device():
    """Everything outside the domain, and every NULL, returns -1 before any device call: the pointers here point nowhere."""
    L = lib()
    p = ctypes.c_void_p(4096)   # stands for a device pointer

    def update(reward=p, done=p, T=4, N=12, K=3, hyper=p, carry=p, stats=p, stride=3, scale=p, eps=1e-8, scratch=p):
        return L.pcc_return_stats_update_pop(reward, done, T, N, K, hyper, carry, stats, stride, scale, eps, scratch, None)

    def norm_(reward=p, T=4, N=12, K=3, scale=p, clip=10.0, out=p):
        return L.pcc_reward_normalise_pop(reward, T, N, K, scale, clip, out, None)

    for call in (update, norm_):
        for kw in ({"T": 0}, {"T": -2}, {"K": 0}, {"K": -1}, {"K": 1025, "N": 2050}, {"N": 13}, {"N": 0}, {"N": -12}, {"reward": None}):
            assert call(**kw) == -1, (call.__name__, kw)
    for kw in ({"eps": -1e-9}, {"eps": float("nan")}, {"stride": 2}, {"stride": 0}, {"stride": -3}, {"done": None}, {"hyper": None},
               {"carry": None}, {"stats": None}, {"scratch": None}):
        assert update(**kw) == -1, kw
    for kw in ({"clip": 0.0}, {"clip": -1.0}, {"clip": float("nan")}, {"scale": None}, {"out": None}):
        assert norm_(**kw) == -1, kw
    # the stand-alone forms: the same answers
    assert L.pcc_return_stats_update(p, p, 0, 12, 0.99, p, p, p, 1e-8, p, None) == -1
    assert L.pcc_return_stats_update(p, p, 4, 0, 0.99, p, p, p, 1e-8, p, None) == -1
    assert L.pcc_return_stats_update(None, p, 4, 12, 0.99, p, p, p, 1e-8, p, None) == -1
    assert L.pcc_return_stats_update(p, None, 4, 12, 0.99, p, p, p, 1e-8, p, None) == -1
    assert L.pcc_return_stats_update(p, p, 4, 12, 0.99, None, p, p, 1e-8, p, None) == -1
    assert L.pcc_return_stats_update(p, p, 4, 12, 0.99, p, None, p, 1e-8, p, None) == -1
    assert L.pcc_return_stats_update(p, p, 4, 12, 0.99, p, p, p, -1.0, p, None) == -1
    assert L.pcc_return_stats_update(p, p, 4, 12, 0.99, p, p, p, 1e-8, None, None) == -1
    assert L.pcc_reward_normalise(p, 0, 12, p, 10.0, p, None) == -1
    assert L.pcc_reward_normalise(p, 4, 12, None, 10.0, p, None) == -1
    assert L.pcc_reward_normalise(p, 4, 12, p, 0.0, p, None) == -1
    assert L.pcc_reward_normalise(p, 4, 12, p, 10.0, None, None) == -1
    assert L.pcc_reward_normalise(None, 4, 12, p, 10.0, p, None) == -1


def test_kernels_use_no_scratch(tmp_path):
    """A build into a temporary file: the three kernels are in the compiler's resource report with 0 bytes of scratch, 0 spilled
    vector registers and at most 64 KB of LDS; the unit is one of its own, and the figures tests/test_population_cpu.py pins for the
    policy kernels are still what the report says."""
    from pcc_rl_amd import build as pbuild
    assert "pcc_rewnorm.hip" in pbuild.UNITS
    out = str(tmp_path / "libpcc_sim_rew.so")
    pbuild.build_library(force=True, out=out)
    res = json.load(open(out + ".resources.json"))
    for name in ("return_walk_kernel", "return_merge_kernel", "reward_normalise_kernel"):
        assert name in res, name
        assert res[name]["scratch"] == 0 and res[name]["vgpr_spills"] == 0, (name, res[name])
        assert res[name]["lds"] <= 64 * 1024, (name, res[name])
    assert sorted(n for n in res if n.startswith(("return_", "reward_"))) == ["return_merge_kernel", "return_walk_kernel", "reward_normalise_kernel"]
    assert (res["ppo_grad_mfma_kernel<30, 32, 16>"]["vgprs"], res["ppo_grad_mfma_kernel<30, 32, 16>"]["lds"]) == (256, 52736)
    assert res["policy_act_fixed_kernel<30, 32, 16>"]["vgprs"] == 87


# ------------------------------------------------------------------------------------------------------------ constructors
class _Env(object):   # what the constructors' argument checks look at, without a simulator behind it
    obs_dim, device, n_senders, n_envs = 30, "cuda:0", 1, 12


class _CpuEnv(_Env):
    device = "cpu"


class _TwoSenders(_Env):
    n_senders = 2


def test_constructors_refuse():
    with pytest.raises(ValueError, match="no CPU path"):
        RewardNormalizer(8, device="cpu")
    with pytest.raises(ValueError, match="do not divide"):
        RewardNormalizer(9, members=2, device="cuda:0")
    with pytest.raises(ValueError, match="do not divide"):
        RewardNormalizer(2050, members=1025, device="cuda:0")
    with pytest.raises(ValueError, match="do not divide"):
        RewardNormalizer(0, device="cuda:0")
    with pytest.raises(ValueError, match="clip"):
        RewardNormalizer(8, clip=0.0, device="cuda:0")
    with pytest.raises(ValueError, match="eps"):
        RewardNormalizer(8, eps=-1.0, device="cuda:0")
    with pytest.raises(ValueError, match="normalize_reward=True.*no CPU path"):
        PPO(_CpuEnv(), normalize_reward=True)
    with pytest.raises(ValueError, match="normalize_reward=True.*one sender"):
        PPO(_TwoSenders(), normalize_reward=True)
    with pytest.raises(ValueError, match="BatchedNetworkEnv"):   # the argument checks as before
        PopulationPPO(_Env(), 3, normalize_reward=True)
