"""Gradient-norm clipping and the non-finite guard, the part that needs no GPU (include/pcc_policy.h: pcc_ppo_minibatch_step_clip_pop;
DESIGN.md section 24): the numpy model of tests/models/grad_clip_model.py held against torch and against an exact sum, the symbol,
every refusal of the host side, the compiler's resource report of the two kernels, and what the constructors refuse."""
import ctypes
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import grad_clip_model as model  # noqa: E402

from pcc_rl_amd import native  # noqa: E402
from pcc_rl_amd.gradclip import GradClip  # noqa: E402
from pcc_rl_amd.native import lib  # noqa: E402
from pcc_rl_amd.ppo import HYPER_COLS, HYPER_NAMES, PPO, PopulationPPO, _hyper_columns, explore_matrix  # noqa: E402

SYMBOL, N_ARGS = "pcc_ppo_minibatch_step_clip_pop", 29
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------- the model alone
def test_the_model_is_clip_grad_norm_and_torch_adam_in_double():
    """Five steps in float64: some clip, some do not.  The model's norm is the ordered sum's, torch's is vector_norm's: they differ by
    the summation order, at most n 2^-53 relative each; the coefficient, the moments and the step inherit a few of those, so the
    parameters are held to 64 n 2^-53 of their own size plus that of the largest possible step, per step."""
    n, lr, limit = 257, 1e-3, 2.0
    g = torch.Generator().manual_seed(1)
    p = torch.nn.Parameter(torch.randn(n, generator=g, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=lr, betas=(model.B1, model.B2), eps=model.EPS)
    q, m, v = p.detach().numpy().copy(), np.zeros(n), np.zeros(n)
    states = []
    for t in range(1, 6):
        grad = torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** float(t - 3)
        p.grad = grad.clone()
        total = torch.nn.utils.clip_grad_norm_([p], limit)
        opt.step()
        q, m, v, state = model.clipped_step64(t, grad.numpy(), m, v, q, lr, limit)
        states.append(state)
        assert (state == model.CLIPPED) == (float(total) > limit - 1e-6)
        tol = t * 64 * n * 2.0 ** -53 * (np.abs(q) + 10.0 * lr)
        assert (np.abs(q - p.detach().numpy()) <= tol).all(), (t, float(np.abs(q - p.detach().numpy()).max()))
        st = opt.state[p]
        assert np.allclose(m, st["exp_avg"].numpy(), rtol=64 * n * 2.0 ** -53, atol=0.0)
        assert np.allclose(v, st["exp_avg_sq"].numpy(), rtol=64 * n * 2.0 ** -53, atol=0.0)
    assert states == [0, 0, 1, 1, 1]   # (norms of about 0.16, 1.6, 16, 160, 1600 against a limit of 2)


@pytest.mark.parametrize("n", [1, 141, 255, 256, 257, 3075, 24963])
def test_the_ordered_sum_is_within_its_bound_of_the_exact_sum(n):
    rng = np.random.default_rng(n)
    for scale in (1.0, 1e-3, 1e4):
        g = (scale * rng.standard_normal(n)).astype(np.float32)
        exact = math.fsum(float(x) * float(x) for x in g)     # (a float32 squared is exact in float64)
        got = model.ordered_sumsq(g)
        assert abs(got - exact) <= n * 2.0 ** -53 * exact, (n, scale, got, exact)
    # the order as stated, on a vector whose sums depend on it: lane j holds p = j, j + 256, ...
    # With e = (1.5 * 2^-27)^2 = 0.5625 ulp(1): 1 + e rounds up to 1 + ulp and again to 1 + 2 ulp, where e + e first gives 1 + ulp.
    ulp, e = 2.0 ** -52, 2.25 * 2.0 ** -54
    g = np.zeros(600, dtype=np.float32)
    g[3], g[259], g[515], g[131] = 1.0, 1.5 * 2.0 ** -27, 1.5 * 2.0 ** -27, 1.5 * 2.0 ** -27
    x = model.lane_sums(g)
    assert x[3] == 1.0 + 2 * ulp and x[131] == e and np.count_nonzero(x) == 2
    assert model.tree(x) == 1.0 + 3 * ulp                    # (j = 3 takes j + 128 = 131 at s = 128: 2.5625 ulp rounds to 3)
    assert math.fsum([1.0, e, e, e]) == 1.0 + 2 * ulp        # ... where the exact sum is 1 + 1.6875 ulp
    assert model.ordered_sumsq(g) == 1.0 + 3 * ulp


def test_the_state_and_coefficient_rules():
    f = np.float32
    assert model.decide(4.0, 0.0, 0.5)[0] == model.GRAD_ONLY and model.decide(float("nan"), 0.0, 0.5)[0] == model.GRAD_ONLY
    assert model.decide(4.0, 0.0, 0.5)[2] == 2.0                          # (the norm is still reported)
    for bad in (float("nan"), float("inf")):
        assert model.decide(bad, 1e-3, 0.5)[:2] == (model.SKIPPED, f(1.0))
    state, c, norm = model.decide(4.0, 1e-3, 0.5)
    assert (state, norm) == (model.CLIPPED, 2.0) and c == f(0.5 / (2.0 + 1e-6))
    assert model.decide(4.0, 1e-3, 0.0)[:2] == (model.APPLIED, f(1.0))    # 0: the guard alone
    assert model.decide(4.0, 1e-3, 1e30)[:2] == (model.APPLIED, f(1.0))
    assert model.decide(4.0, 1e-3, 2.0)[0] == model.CLIPPED               # (2 / (2 + 1e-6) < 1, as clip_grad_norm_ has it)
    assert model.decide(4.0, 1e-3, 2.0 + 2e-6)[0] == model.APPLIED
    assert model.decide(0.0, 1e-3, 0.5)[:2] == (model.APPLIED, f(1.0))    # a zero gradient: 0.5 / 1e-6 is no clip
    row = [0.0] * 8
    for sumsq, lr, want in ((4.0, 1e-3, 1), (1e-2, 1e-3, 0), (float("nan"), 1e-3, 2), (9.0, 0.0, 3), (1.0, 1e-3, 1)):
        assert model.accumulate(row, sumsq, lr, 0.5) == want
    assert row[4:] == [3.0, 2.0, 1.0, 3.0] and row[:4] == [1.0, 1.0, float(f(0.5 / (1.0 + 1e-6))), 1.0]


def test_hyper_column_five():
    assert HYPER_NAMES[5] == "max_grad_norm" and HYPER_COLS == 8
    rows = _hyper_columns(2, lr=1e-3, clip=0.2, ent_coef=0.01, gamma=0.99, lam=0.95, max_grad_norm=[0.5, 2.0])
    assert [r[5] for r in rows] == [0.5, 2.0] and all(r[6:] == [0.0, 0.0] and len(r) == 8 for r in rows)
    ex = explore_matrix(explore=("max_grad_norm",), bounds={"max_grad_norm": (0.1, 10.0)})
    assert ex[5] == [0.8, 1.2, 0.1, 10.0] and ex[0] == [1.0, 1.0, -float("inf"), float("inf")]
    assert explore_matrix()[5] == [1.0, 1.0, -float("inf"), float("inf")]     # (by default a replaced member inherits its parent's)


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "pcc_policy.h")).read()
    decl = re.search(r"\nint %s\((.*?)\);" % SYMBOL, header, re.S)
    assert decl is not None
    assert len(decl.group(1).split(",")) == N_ARGS
    assert "max_grad_norm" in header
    assert SYMBOL in native.SYMBOLS
    L = lib()
    assert hasattr(L, SYMBOL)
    assert len(getattr(L, SYMBOL).argtypes) == N_ARGS == len(L.pcc_ppo_minibatch_step_pop.argtypes) + 3


def test_refusals_need_no_device():
    """Everything pcc_ppo_minibatch_step_pop refuses, a NULL grad_out / hyper_grad / clip and a short clip row return -1, a shape
    outside pcc_ppo_supported -2, before any device call: the pointers here point nowhere."""
    L = lib()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)   # stand for device pointers

    def step(obs=p, act=p, logp=p, adv=p, ret=p, perm=p, perm_stride=256, start=17, count=200, D=30, h1=32, h2=16, params=p, m=p, v=p,
             stride=3136, K=3, hyper=p, t=1, scratch=p, grad=p, stats=p, hyper_grad=q, clip=p, clip_stride=8):
        return L.pcc_ppo_minibatch_step_clip_pop(obs, act, logp, adv, ret, perm, perm_stride, start, count, D, h1, h2, params, m, v, stride, K,
                                                 hyper, t, 0.9, 0.999, 1e-5, scratch, grad, stats, hyper_grad, clip, clip_stride, None)

    for kw in ({"obs": None}, {"act": None}, {"logp": None}, {"adv": None}, {"ret": None}, {"perm": None}, {"params": None}, {"scratch": None},
               {"hyper": None}, {"count": 0}, {"count": -5}, {"start": -1}, {"m": None}, {"v": None}, {"t": 0}, {"t": -1}, {"K": 0}, {"K": -1},
               {"K": 1025}, {"perm_stride": -1}, {"stride": 3075}, {"stride": 3072}, {"stride": 0}, {"stride": -64}, {"stride": 3136 + 32},
               {"grad": None}, {"hyper_grad": None}, {"clip": None}, {"clip_stride": 7}, {"clip_stride": 0}, {"clip_stride": -8},
               {"hyper_grad": p}):
        assert step(**kw) == -1, kw
    for kw in ({"D": 0}, {"D": 129}, {"D": -1}, {"h1": 0}, {"h1": 65}, {"h2": 0}, {"h2": 65}):
        assert step(**kw) == -2, kw
    assert step(D=129, grad=None) == -1 and step(D=129, clip_stride=7) == -1   # (the NULLs and the row length come first)
    # ... and where the unclipped entry answers, it answers the same
    for kw in ({"count": 0}, {"K": 1025}, {"stride": 3072}, {"t": 0}, {"perm": None}, {"D": 129}, {"h1": 65}):
        a = dict(dict(perm=p, count=200, D=30, h1=32, stride=3136, K=3, t=1), **kw)
        want = L.pcc_ppo_minibatch_step_pop(p, p, p, p, p, a["perm"], 256, 17, a["count"], a["D"], a["h1"], 16, p, p, p, a["stride"], a["K"], p,
                                            a["t"], 0.9, 0.999, 1e-5, p, p, p, None)
        assert want in (-1, -2) and step(**kw) == want, kw


def test_kernels_use_no_scratch_and_the_older_kernels_keep_their_figures(tmp_path):
    """A build into a temporary file: the two kernels are in the compiler's resource report with 0 bytes of scratch, 0 spilled
    vector registers and at most 64 KB of LDS; the unit is one of its own, and the figures the suite pins for the older kernels are
    still what the report says."""
    from pcc_rl_amd import build as pbuild
    assert "pcc_gradclip.hip" in pbuild.UNITS and pbuild.UNITS.count("pcc_gradclip.hip") == 1
    out = str(tmp_path / "libpcc_sim_clip.so")
    pbuild.build_library(force=True, out=out)
    res = json.load(open(out + ".resources.json"))
    for name in ("clip_adam_kernel", "clip_hyper_kernel"):
        assert name in res, name
        assert res[name]["scratch"] == 0 and res[name]["vgpr_spills"] == 0, (name, res[name])
        assert res[name]["lds"] <= 64 * 1024, (name, res[name])
    assert res["clip_adam_kernel"]["lds"] == 256 * 8        # the tree over 256 doubles, nothing else
    assert sorted(n for n in res if n.startswith("clip_")) == ["clip_adam_kernel", "clip_hyper_kernel"]
    for unit in pbuild.UNITS:
        if unit != "pcc_gradclip.hip":
            assert "clip_adam_kernel" not in open(os.path.join(pbuild.CSRC, unit)).read(), unit
    assert (res["ppo_grad_mfma_kernel<30, 32, 16>"]["vgprs"], res["ppo_grad_mfma_kernel<30, 32, 16>"]["lds"]) == (256, 52736)
    assert res["policy_act_fixed_kernel<30, 32, 16>"]["vgprs"] == 87
    assert res["ppo_adam_kernel"]["scratch"] == 0 and res["diag_walk_kernel"]["scratch"] == 0


# ------------------------------------------------------------------------------------------------------------ constructors
class _Env(object):   # what the constructors' argument checks look at, without a simulator behind it
    obs_dim, device, n_senders, n_envs = 30, "cuda:0", 1, 12


class _CpuEnv(_Env):
    device = "cpu"


def test_constructors_refuse():
    with pytest.raises(ValueError, match="no CPU path"):
        GradClip(3136, device="cpu")
    for members in (0, 1025):
        with pytest.raises(ValueError, match="members"):
            GradClip(3136, members, device="cuda:0")
    with pytest.raises(ValueError, match="param_stride"):
        GradClip(3075, device="cuda:0")
    for bad in (-1, -1e-9, float("nan"), float("inf"), [0.5, -1.0, 0.5]):
        with pytest.raises(ValueError, match="max_grad_norm"):
            PPO(_Env(), max_grad_norm=bad) if not isinstance(bad, list) else PopulationPPO(_Env(), 3, max_grad_norm=bad)
        if not isinstance(bad, list):
            with pytest.raises(ValueError, match="max_grad_norm"):
                PopulationPPO(_Env(), 3, max_grad_norm=bad)
    for wrong in ([0.5, 0.5], [0.5] * 4, []):   # one value per member, or a scalar
        with pytest.raises(ValueError, match="max_grad_norm has"):
            PopulationPPO(_Env(), 3, max_grad_norm=wrong)
    with pytest.raises(ValueError, match="max_grad_norm has"):
        PPO(_Env(), max_grad_norm=[0.5, 0.5])
    with pytest.raises(ValueError, match="needs the fused update"):
        PPO(_Env(), max_grad_norm=0.5, fused_update=False)
    with pytest.raises(ValueError, match="no CPU path"):
        PPO(_CpuEnv(), max_grad_norm=0.5)
    with pytest.raises(ValueError, match="no CPU path"):
        PopulationPPO(_CpuEnv(), 3, max_grad_norm=0.5)
    with pytest.raises(ValueError, match="BatchedNetworkEnv"):        # the argument checks as before
        PopulationPPO(_Env(), 3, max_grad_norm=0.5)
