"""Update diagnostics and the KL guard, the part that needs no GPU (include/pcc_policy.h: pcc_policy_act_rows_pop,
pcc_update_diag_pop and its stand-alone form): the numpy model of tests/models/update_diag_model.py held
against itself, every case of the GPU table against its clip margin, the four symbols, every refusal of the host side, the compiler's
resource report of the two kernels, and what the constructors refuse."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import update_diag_model as model  # noqa: E402

from pcc_rl_amd import native  # noqa: E402
from pcc_rl_amd.native import lib  # noqa: E402
from pcc_rl_amd.ppo import PPO, PopulationPPO  # noqa: E402
from pcc_rl_amd.updiag import UpdateDiagnostics  # noqa: E402

DIAG_SYMBOLS = {"pcc_policy_act_rows_pop": 13, "pcc_update_diag_scratch_doubles": 4, "pcc_update_diag_pop": 21, "pcc_update_diag": 14}
PART = 9   # doubles per workgroup of the walk (csrc/pcc_updiag.hip: kDiagPart)


# ---------------------------------------------------------------------------------------------------------- the model alone
def test_k_is_never_negative_and_small_shifts_give_half_d_squared():
    d = np.concatenate([np.linspace(-30.0, 8.0, 2001), [0.0, 1e-9, -1e-9, 1e-300]])
    k = np.expm1(d) - d
    assert (k >= 0.0).all()
    rng = np.random.default_rng(3)
    for shift in (1e-3, 1e-2):
        for ls in model.LOG_STDS:
            mean = rng.standard_normal((6, 500)).astype(np.float32)
            act = (mean + np.exp(ls) * rng.standard_normal((6, 500))).astype(np.float32)
            lo = model.logp32(act, mean, ls)
            new = (mean + np.float32(shift)).astype(np.float32)
            ref = model.reference(act, lo, new, act, act, ls, 0.2)
            d, _ = model.log_ratio(act, lo, new, ls)
            assert ref["approx_kl"] >= 0.0
            assert abs(ref["approx_kl"] - float((d * d).mean()) / 2.0) <= 0.05 * ref["approx_kl"], (shift, ls)
            # the Gaussians' own KL: shift^2 / (2 sigma^2), up to the sampling error of the mean of eps^2 (n = 3000)
            assert abs(ref["approx_kl"] / (shift * shift / (2.0 * np.exp(2.0 * ls))) - 1.0) < 0.15, (shift, ls)


def test_the_reference_row():
    act = np.array([[0.0, 1.0], [2.0, 3.0], [9.0, 9.0]], dtype=np.float32)
    mean = np.array([[0.0, 1.0], [2.0, 2.0], [0.0, 0.0]], dtype=np.float32)
    lo = model.logp32(act, act, 0.0)   # (the rollout's mean was the action itself: z = 0)
    ret = np.array([[1.0, 2.0], [3.0, 4.0], [7.0, 7.0]], dtype=np.float32)
    val = np.array([[1.0, 1.0], [3.0, 3.0], [0.0, 0.0]], dtype=np.float32)
    r = model.reference(act, lo, mean, ret, val, 0.0, 0.2, row_step=2)   # rows 0 and 2
    d = np.array([0.0, 0.0, -40.5, -40.5]) + (np.float64(np.float32(model.HALF_LOG_2PI)) - model.HALF_LOG_2PI)
    assert r["count"] == 4.0 and r["clipped"] == 2 and r["clip_fraction"] == 0.5 and r["nonfinite"] == 0.0
    assert abs(r["max_abs_log_ratio"] - 40.5) < 1e-6
    assert abs(r["approx_kl"] - float((np.expm1(d) - d).mean())) < 1e-12
    assert r["var_ret"] == np.var([1.0, 2.0, 7.0, 7.0]) and r["var_resid"] == np.var([0.0, 1.0, 7.0, 7.0])
    assert r["explained_variance"] == 1.0 - r["var_resid"] / r["var_ret"]
    # a constant return: no variance to explain
    assert np.isnan(model.reference(act, lo, mean, np.full_like(ret, 0.1), val, 0.0, 0.2)["explained_variance"])
    # a NaN mean: the KL is NaN, the sample is counted, the maximum does not see it
    bad = mean.copy()
    bad[1, 0] = np.nan
    r = model.reference(act, lo, bad, ret, val, 0.0, 0.2)
    assert np.isnan(r["approx_kl"]) and r["nonfinite"] == 1.0 and r["max_abs_log_ratio"] == pytest.approx(40.5, abs=1e-6)
    assert r["clipped"] == 3   # (the NaN sample is not clipped: the comparison is false)


def test_the_decision_rule():
    hyper = np.arange(1, 41, dtype=np.float32).reshape(5, 8)
    kl = np.array([0.01, 0.04, np.nan, 0.03, 0.5])
    stop, live = model.decide([0, 0, 0, 2, 0], kl, 0.03, 3, hyper)
    assert stop.tolist() == [0, 3, 3, 2, 3]               # (0.03 <= 0.03 would not stop; the sticky 2 stays 2; NaN stops)
    assert live[:, 0].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and np.array_equal(live[:, 1:], hyper[:, 1:])
    for limit in (0.0, -1.0):                             # diagnostics only: nobody stops, NaN included
        stop, live = model.decide([0, 0, 0, 2, 0], kl, limit, 3, hyper)
        assert stop.tolist() == [0, 0, 0, 2, 0] and live[:, 0].tolist() == [1.0, 9.0, 17.0, 0.0, 33.0]
    stop, _ = model.decide([0], np.array([0.03]), 0.03, 1, hyper[:1])
    assert stop.tolist() == [0]


@pytest.mark.parametrize("name", sorted(model.CASES))
def test_the_gpu_cases_keep_their_clip_margin(name):
    """The inputs are chosen here, on the CPU: no sample of any member sits so close to the clip range that a device within delta
    of the reference could count it differently; and the bounds are finite, positive and small next to what they bound."""
    case = model.make_case(name)
    assert (case["T"], case["n_m"], case["K"]) == model.CASES[name][:3]
    for m in range(case["K"]):
        cols = [model.member(case, m, k) for k in ("act", "logp_old", "mean_new")]
        assert model.clip_margin_ok(*cols, case["log_std"][m], case["clip"], case["row_step"]), (name, m)
        ref, b = model.member_reference(case, m)
        n_rows = (case["T"] - 1) // case["row_step"] + 1
        assert ref["count"] == n_rows * case["n_m"] and ref["nonfinite"] == 0.0
        assert 0.0 < b["approx_kl"] < max(1e-9, 1e-2 * ref["approx_kl"]) or ref["approx_kl"] < 1e-9, (name, m, b, ref)
        assert 0.0 < b["max_abs_log_ratio"] < 1e-3
        if case["kind"] == "constant":
            assert np.isnan(ref["explained_variance"]) and ref["var_ret"] == 0.0
        elif ref["count"] > 1:
            assert b["explained_variance"] < 1e-6 and b["var_ret"] < 1e-6 and b["var_resid"] < 1e-6


def test_the_bound_covers_a_float32_restatement():
    """The log-ratio recomputed operation by operation in numpy float32 stays within delta of the float64 one."""
    worst = 0.0
    for name in sorted(model.CASES):
        case = model.make_case(name)
        for m in range(case["K"]):
            act, lo, new = (model.member(case, m, k) for k in ("act", "logp_old", "mean_new"))
            d32 = (model.logp32(act, new, case["log_std"][m]) - lo).astype(np.float32)
            d, z = model.log_ratio(act, lo, new, case["log_std"][m])
            dl = model.deltas(z, lo, case["log_std"][m])
            assert (np.abs(d32.astype(np.float64) - d) <= dl).all(), (name, m)
            worst = max(worst, float((np.abs(d32.astype(np.float64) - d) / dl).max()))
    print("the float32 restatement uses at most %.2f %% of delta" % (100.0 * worst))


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_four_symbols_are_exported():
    L = lib()
    for s, n_args in DIAG_SYMBOLS.items():
        assert s in native.SYMBOLS, s
        assert hasattr(L, s), s
        assert len(getattr(L, s).argtypes) == n_args, s


def test_scratch_size():
    L = lib()
    for T, step, N, K, groups in ((1, 1, 1, 1, 1), (5, 1, 771, 3, 2), (64, 8, 65536, 8, 32), (64, 1, 65536, 1, 256), (400, 1, 64, 1, 1),
                                  (1, 7, 1024, 1024, 1), (3, 2, 256, 1, 1), (3, 1, 257, 1, 2), (7, 9, 8198, 2, 17)):
        assert L.pcc_update_diag_scratch_doubles(T, step, N, K) == groups * K * PART, (T, step, N, K)
    for T, step, N, K in ((0, 1, 8, 1), (-1, 1, 8, 1), (4, 0, 8, 1), (4, -1, 8, 1), (4, 1, 8, 0), (4, 1, 2050, 1025), (4, 1, 9, 2),
                          (4, 1, 0, 1), (4, 1, -8, 1)):
        assert L.pcc_update_diag_scratch_doubles(T, step, N, K) == -1, (T, step, N, K)


def test_refusals_need_no_device():
    """Everything outside the domain, and every NULL, returns -1 (an observation length outside 1 .. 128: -2) before any device
    call: the pointers here point nowhere."""
    L = lib()
    p = ctypes.c_void_p(4096)   # stands for a device pointer

    def diag(act=p, logp=p, mean=p, ret=p, val=p, T=4, step=1, N=12, K=3, params=p, stride=3136, index=1537, hyper=p, limit=0.03, epoch=1,
             out=p, out_stride=8, stop=p, live=p, scratch=p):
        return L.pcc_update_diag_pop(act, logp, mean, ret, val, T, step, N, K, params, stride, index, hyper, limit, epoch, out, out_stride,
                                     stop, live, scratch, None)

    for kw in ({"T": 0}, {"T": -2}, {"step": 0}, {"step": -1}, {"N": 0}, {"N": -12}, {"K": 0}, {"K": -1}, {"K": 1025, "N": 2050}, {"N": 13},
               {"out_stride": 7}, {"out_stride": 0}, {"out_stride": -8}, {"epoch": 0}, {"epoch": -1}, {"index": -1}, {"index": 3136},
               {"index": 1 << 40}, {"stride": 3075}, {"stride": 0}, {"stride": -64}, {"act": None}, {"logp": None}, {"mean": None},
               {"ret": None}, {"val": None}, {"params": None}, {"hyper": None}, {"out": None}, {"scratch": None}, {"stop": None},
               {"live": None}):
        assert diag(**kw) == -1, kw

    def alone(act=p, logp=p, mean=p, ret=p, val=p, T=4, step=1, N=12, params=p, index=1537, clip=0.2, out=p, scratch=p):
        return L.pcc_update_diag(act, logp, mean, ret, val, T, step, N, params, index, clip, out, scratch, None)

    for kw in ({"T": 0}, {"step": 0}, {"N": 0}, {"N": -1}, {"index": -1}, {"act": None}, {"logp": None}, {"mean": None}, {"ret": None},
               {"val": None}, {"params": None}, {"out": None}, {"scratch": None}):
        assert alone(**kw) == -1, kw

    def rows(obs=p, T=4, step=1, N=12, D=30, params=p, stride=3136, K=3, h1=32, h2=16, mean=p, value=p):
        return L.pcc_policy_act_rows_pop(obs, T, step, N, D, params, stride, K, h1, h2, mean, value, None)

    for kw in ({"T": 0}, {"T": -1}, {"step": 0}, {"step": -3}, {"obs": None}, {"params": None}, {"N": 0}, {"N": 13}, {"K": 0}, {"K": 1025, "N": 2050},
               {"h1": 0}, {"h1": 65}, {"h2": 0}, {"h2": 65}, {"stride": 3075}, {"stride": 3072}, {"stride": 0}):
        assert rows(**kw) == -1, kw
    for kw in ({"D": 0}, {"D": 129}, {"D": -1}):
        assert rows(**kw) == -2, kw
    assert rows(T=0, D=129) == -1   # (the rows come first)


def test_kernels_use_no_scratch(tmp_path):
    """A build into a temporary file: the two kernels are in the compiler's resource report with 0 bytes of scratch, 0 spilled
    vector registers and at most 64 KB of LDS; the unit is one of its own, and the figures tests/test_population_cpu.py pins for the
    policy kernels are still what the report says."""
    from pcc_rl_amd import build as pbuild
    assert "pcc_updiag.hip" in pbuild.UNITS
    out = str(tmp_path / "libpcc_sim_diag.so")
    pbuild.build_library(force=True, out=out)
    res = json.load(open(out + ".resources.json"))
    for name in ("diag_walk_kernel", "diag_merge_kernel"):
        assert name in res, name
        assert res[name]["scratch"] == 0 and res[name]["vgpr_spills"] == 0, (name, res[name])
        assert res[name]["lds"] <= 64 * 1024, (name, res[name])
    assert sorted(n for n in res if n.startswith("diag_")) == ["diag_merge_kernel", "diag_walk_kernel"]
    assert (res["ppo_grad_mfma_kernel<30, 32, 16>"]["vgprs"], res["ppo_grad_mfma_kernel<30, 32, 16>"]["lds"]) == (256, 52736)
    assert res["policy_act_fixed_kernel<30, 32, 16>"]["vgprs"] == 87
    assert res["ppo_adam_kernel"]["scratch"] == 0 and res["return_walk_kernel"]["scratch"] == 0


# ------------------------------------------------------------------------------------------------------------ constructors
class _Env(object):   # what the constructors' argument checks look at, without a simulator behind it
    obs_dim, device, n_senders, n_envs = 30, "cuda:0", 1, 12


class _CpuEnv(_Env):
    device = "cpu"


class _TwoSenders(_Env):
    n_senders = 2


def test_constructors_refuse():
    with pytest.raises(ValueError, match="no CPU path"):
        UpdateDiagnostics(8, device="cpu")
    with pytest.raises(ValueError, match="do not divide"):
        UpdateDiagnostics(9, members=2, device="cuda:0")
    with pytest.raises(ValueError, match="do not divide"):
        UpdateDiagnostics(2050, members=1025, device="cuda:0")
    with pytest.raises(ValueError, match="do not divide"):
        UpdateDiagnostics(0, device="cuda:0")
    with pytest.raises(ValueError, match="row_step"):
        UpdateDiagnostics(8, device="cuda:0", row_step=0)
    for kw in ({"diagnostics": True}, {"target_kl": 0.02}):
        with pytest.raises(ValueError, match="no CPU path"):
            PPO(_CpuEnv(), **kw)
        with pytest.raises(ValueError, match="one sender"):
            PPO(_TwoSenders(), **kw)
        with pytest.raises(ValueError, match="needs the fused update"):   # the framework path has no diagnostics
            PPO(_Env(), fused_update=False, **kw)
        with pytest.raises(ValueError, match="BatchedNetworkEnv"):        # the argument checks as before
            PopulationPPO(_Env(), 3, **kw)
    with pytest.raises(ValueError, match="target_kl"):
        PPO(_Env(), target_kl=0.0)
    with pytest.raises(ValueError, match="target_kl"):
        PPO(_Env(), target_kl=float("nan"))
    with pytest.raises(ValueError, match="diag_rows"):
        PPO(_Env(), diagnostics=True, diag_rows=0)
