"""Observation normalisation, the part that needs no GPU (include/pcc_policy.h: pcc_obs_stats_update_pop, pcc_obs_normalise_pop
and their stand-alone forms): the five symbols, every refusal of the host side, the compiler's resource report
of the three kernels, what the trainers' constructors refuse, the exported policy -- and a numpy restatement of the contract
(Chan's merge, norm from stats, the normalise formula), which tests/test_obs_norm.py holds the device against."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from pcc_rl_amd import native
from pcc_rl_amd.export import export_policy, load_policy
from pcc_rl_amd.native import lib
from pcc_rl_amd.ppo import PPO, MlpPolicy, PopulationPPO

OBS_SYMBOLS = {"pcc_obs_stats_scratch_doubles": 4, "pcc_obs_stats_update_pop": 11, "pcc_obs_normalise_pop": 8,
               "pcc_obs_stats_update": 9, "pcc_obs_normalise": 7}
U = 2.0 ** -53   # float64's unit roundoff


# ------------------------------------------------------------------------------------------ the contract, restated in numpy
def batch_moments(x):
    """(n, mean, m2) of the rows of x [n][D], float64 two-pass: the reference of every moments check."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=0)
    return x.shape[0], mean, ((x - mean) ** 2).sum(axis=0)


def chan_merge(a, b):
    """(n_a, mean_a, m2_a) with (n_b, mean_b, m2_b) merged in, the header's formula; an empty a becomes b."""
    (na, ma, qa), (nb, mb, qb) = a, b
    if na == 0:
        return float(nb), np.array(mb, dtype=np.float64), np.array(qb, dtype=np.float64)
    n = na + nb
    d = mb - ma
    return float(n), ma + d * nb / n, qa + qb + d * d * na * nb / n


def member_rows(obs, m, K):
    """Member m's rows of obs [T][N][D] (or [N][D]) as [n][D]: its columns, step by step."""
    n_m = obs.shape[-2] // K
    return obs[..., m * n_m:(m + 1) * n_m, :].reshape(-1, obs.shape[-1])


def update_stats(stats, obs, K):
    """stats [K][stride] after pcc_obs_stats_update_pop on obs [T][N][D]; the padding stays."""
    D = obs.shape[-1]
    out = np.array(stats, dtype=np.float64)
    for m in range(K):
        row = out[m]
        n, mean, m2 = chan_merge((row[0], row[1:1 + D].copy(), row[1 + D:1 + 2 * D].copy()), batch_moments(member_rows(obs, m, K)))
        row[0], row[1:1 + D], row[1 + D:1 + 2 * D] = n, mean, m2
    return out


def norm_from_stats(stats, D, eps):
    """norm [K][2 D] float32 from stats: float64 arithmetic, rounded to float32 once."""
    stats = np.asarray(stats, dtype=np.float64)
    count, mean, m2 = stats[:, :1], stats[:, 1:1 + D], stats[:, 1 + D:1 + 2 * D]
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = 1.0 / np.sqrt(m2 / count + np.float64(eps))
    return np.concatenate([mean.astype(np.float32), scale.astype(np.float32)], axis=1)


def normalise(obs, norm, K, clip):
    """out [N][D] float32: three float32 operations per element, member m's columns with row m of norm."""
    obs = np.asarray(obs, dtype=np.float32)
    N, D = obs.shape
    n_m = N // K
    shift = np.repeat(norm[:, :D], n_m, axis=0).astype(np.float32)
    scale = np.repeat(norm[:, D:], n_m, axis=0).astype(np.float32)
    c = np.float32(clip)
    with np.errstate(over="ignore", invalid="ignore"):   # (a product beyond float32 is +-inf, and clipped)
        return np.fmin(np.fmax((obs - shift) * scale, -c), c).astype(np.float32)


def moment_bounds(n, max_abs):
    """The allowed |mean - want| and |m2 / count - want| for n rows: the worst case of recursive summation in float64, with a
    factor 8 for the merge arithmetic."""
    return 8.0 * n * U * max_abs, 8.0 * n * U * max_abs * max_abs


INPUT_KINDS = ("unit", "offset", "wide")   # N(0, 1), N(1e4, 1), N(0, 3e3)


def make_input(kind, shape, rng):
    loc, sd = {"unit": (0.0, 1.0), "offset": (1e4, 1.0), "wide": (0.0, 3e3)}[kind]
    return (loc + sd * rng.standard_normal(shape)).astype(np.float32)


def test_the_restatement_merges_like_a_two_pass():
    rng = np.random.default_rng(1)
    D = 7
    for kinds in (("unit",) * 3, ("offset",) * 3, ("wide",) * 3, INPUT_KINDS):
        for sizes in ((1, 1, 1), (5, 1285, 28693), (1285, 5, 1)):
            parts = [make_input(k, (n, D), rng) for k, n in zip(kinds, sizes)]
            acc = (0.0, np.zeros(D), np.zeros(D))
            for p in parts:
                acc = chan_merge(acc, batch_moments(p))
            whole = np.concatenate(parts)
            n, mean, m2 = batch_moments(whole)
            b_mean, b_var = moment_bounds(n, float(np.abs(whole).max()))
            assert acc[0] == n
            assert np.abs(acc[1] - mean).max() <= b_mean, (kinds, sizes)
            assert np.abs(acc[2] / n - m2 / n).max() <= b_var, (kinds, sizes)


def test_the_restatement_normalises():
    norm = np.array([[1.0, -2.0, 0.5, 4.0], [0.0, 0.0, 1.0, 1.0]], dtype=np.float32)   # two members, D = 2
    obs = np.array([[2.0, 0.0], [1e9, -1e9], [3.0, -7.0], [np.nan, 50.0]], dtype=np.float32)
    got = normalise(obs, norm, 2, 5.0)
    assert got.tolist() == [[0.5, 5.0], [5.0, -5.0], [3.0, -5.0], [-5.0, 5.0]]   # (fmax(NaN, -clip) = -clip, like fmaxf)
    st = np.array([[4.0, 1.5, 8.0, 16.0, 0.0, 99.0]])                                    # count 4, D = 2, one padding double
    n = norm_from_stats(st, 2, 0.0)
    assert n.dtype == np.float32 and n.tolist() == [[1.5, 8.0, 0.5, np.inf]]


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_five_symbols_are_exported():
    L = lib()
    for s, n_args in OBS_SYMBOLS.items():
        assert s in native.SYMBOLS, s
        assert hasattr(L, s), s
        assert len(getattr(L, s).argtypes) == n_args, s


def test_scratch_size():
    L = lib()
    for T, N, D, K in ((1, 1, 1, 1), (5, 771, 30, 3), (64, 65536, 30, 8), (64, 65536, 30, 1), (3, 64, 128, 1), (1, 1024, 1, 1024)):
        assert L.pcc_obs_stats_scratch_doubles(T, N, D, K) > 0, (T, N, D, K)
    for T, N, D, K in ((0, 8, 30, 1), (-1, 8, 30, 1), (4, 8, 0, 1), (4, 8, 129, 1), (4, 8, 30, 0), (4, 2050, 30, 1025), (4, 9, 30, 2),
                       (4, 0, 30, 1)):
        assert L.pcc_obs_stats_scratch_doubles(T, N, D, K) == -1, (T, N, D, K)


def test_refusals_need_no_device():
    """Everything outside the domain, and every NULL, returns -1 before any device call: the pointers here point nowhere."""
    L = lib()
    p = ctypes.c_void_p(4096)   # stands for a device pointer

    def update(obs=p, T=4, N=12, D=30, K=3, stats=p, stride=61, norm=p, eps=1e-8, scratch=p):
        return L.pcc_obs_stats_update_pop(obs, T, N, D, K, stats, stride, norm, eps, scratch, None)

    def norm_(obs=p, N=12, D=30, K=3, norm=p, clip=10.0, out=p):
        return L.pcc_obs_normalise_pop(obs, N, D, K, norm, clip, out, None)

    for call in (update, norm_):
        for kw in ({"D": 0}, {"D": 129}, {"D": -3}, {"K": 0}, {"K": 1025, "N": 2050}, {"N": 13}, {"N": 0}, {"obs": None}):
            assert call(**kw) == -1, (call.__name__, kw)
    for kw in ({"T": 0}, {"T": -2}, {"eps": -1e-9}, {"eps": float("nan")}, {"stride": 60}, {"stride": 0}, {"stats": None}, {"scratch": None}):
        assert update(**kw) == -1, kw
    for kw in ({"clip": 0.0}, {"clip": -1.0}, {"clip": float("nan")}, {"norm": None}, {"out": None}):
        assert norm_(**kw) == -1, kw
    # the stand-alone forms: the same answers
    assert L.pcc_obs_stats_update(p, 0, 12, 30, p, p, 1e-8, p, None) == -1
    assert L.pcc_obs_stats_update(p, 4, 12, 129, p, p, 1e-8, p, None) == -1
    assert L.pcc_obs_stats_update(None, 4, 12, 30, p, p, 1e-8, p, None) == -1
    assert L.pcc_obs_stats_update(p, 4, 12, 30, None, p, 1e-8, p, None) == -1
    assert L.pcc_obs_stats_update(p, 4, 12, 30, p, p, -1.0, p, None) == -1
    assert L.pcc_obs_stats_update(p, 4, 12, 30, p, p, 1e-8, None, None) == -1
    assert L.pcc_obs_normalise(p, 12, 0, p, 10.0, p, None) == -1
    assert L.pcc_obs_normalise(p, 12, 30, None, 10.0, p, None) == -1
    assert L.pcc_obs_normalise(p, 12, 30, p, 0.0, p, None) == -1
    assert L.pcc_obs_normalise(p, 12, 30, p, 10.0, None, None) == -1
    assert L.pcc_obs_normalise(None, 12, 30, p, 10.0, p, None) == -1


def test_kernels_use_no_scratch(tmp_path):
    """A build into a temporary file: the three kernels are in the compiler's resource report with 0 bytes of scratch, 0 spilled
    vector registers and at most 64 KB of LDS; the unit is one of its own, and the figures tests/test_population_cpu.py pins for the
    policy kernels are still what the report says."""
    from pcc_rl_amd import build as pbuild
    assert "pcc_obsnorm.hip" in pbuild.UNITS
    out = str(tmp_path / "libpcc_sim_obs.so")
    pbuild.build_library(force=True, out=out)
    res = json.load(open(out + ".resources.json"))
    for name in ("obs_moments_kernel", "obs_merge_kernel", "obs_normalise_kernel"):
        assert name in res, name
        assert res[name]["scratch"] == 0 and res[name]["vgpr_spills"] == 0, (name, res[name])
        assert res[name]["lds"] <= 64 * 1024, (name, res[name])
    assert sorted(n for n in res if n.startswith("obs_")) == ["obs_merge_kernel", "obs_moments_kernel", "obs_normalise_kernel"]
    assert not [n for n in res if n.startswith("obs_") and any(s in n for s in ("policy_act", "ppo_grad", "ppo_adam", "gae_", "_pop_kernel", "_body"))]
    assert (res["ppo_grad_mfma_kernel<30, 32, 16>"]["vgprs"], res["ppo_grad_mfma_kernel<30, 32, 16>"]["lds"]) == (256, 52736)
    assert res["policy_act_fixed_kernel<30, 32, 16>"]["vgprs"] == 87


# ------------------------------------------------------------------------------------------------------------ the trainers
class _Env(object):   # what the constructors' argument checks look at, without a simulator behind it
    obs_dim, device, n_senders, n_envs = 30, "cuda:0", 1, 12


class _Grouped(_Env):
    groups = ()


def test_constructors_refuse():
    with pytest.raises(ValueError, match="policy_in_step.*raw observation rows"):
        PPO(_Env(), policy_in_step=True, normalize_obs=True)
    with pytest.raises(ValueError, match="GroupedNetworkEnv.*raw observation rows"):
        PPO(_Grouped(), normalize_obs=True)
    with pytest.raises(ValueError, match="GroupedNetworkEnv.*raw observation rows"):
        PopulationPPO(_Grouped(), 3, normalize_obs=True)
    with pytest.raises(ValueError, match="BatchedNetworkEnv"):   # past the normalisation checks: the argument checks as before
        PopulationPPO(_Env(), 3, normalize_obs=True)


# --------------------------------------------------------------------------------------------------------------- export
def test_exported_policy_normalises(tmp_path):
    torch.manual_seed(3)
    D = 30
    policy = MlpPolicy(D, 1, (32, 16))
    g = torch.Generator().manual_seed(5)
    shift = torch.randn(D, generator=g) * 100.0
    scale = torch.rand(D, generator=g) * 2.0 + 1e-3
    clip = 4.0
    ob = torch.randn((33, D), generator=g) * 300.0 + shift          # many values beyond the clip on both sides
    with_norm, without = str(tmp_path / "with"), str(tmp_path / "without")
    export_policy(policy, with_norm, obs_norm=(shift, scale, clip))
    export_policy(policy, without)
    with torch.no_grad():
        x = torch.clamp((ob - shift) * scale, -clip, clip)
        assert (x.abs() == clip).any() and (x.abs() < clip).any()
        want, plain = policy.pi(x), policy.pi(ob)
    got = torch.from_numpy(load_policy(with_norm)(ob.numpy()))
    assert torch.equal(got, want)
    assert torch.equal(torch.from_numpy(load_policy(with_norm)(ob[4].numpy())), want[4])   # one observation
    assert torch.equal(torch.from_numpy(load_policy(without)(ob.numpy())), plain)          # as today
    assert not torch.equal(want, plain)
    sig = json.load(open(os.path.join(with_norm, "signature.json")))
    assert sig["obs_norm"] is True and sig["inputs"] == {"ob": [None, D]}
    sig0 = json.load(open(os.path.join(without, "signature.json")))
    assert "obs_norm" not in sig0 and {k: v for k, v in sig.items() if k != "obs_norm"} == sig0
    names = [n for n, _ in torch.jit.load(os.path.join(without, "policy.pt")).named_buffers()]
    assert names == []                                                                      # no normaliser in the plain module
