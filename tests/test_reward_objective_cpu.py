"""Reward objectives, the part that needs no GPU (include/pcc_policy.h: pcc_reward_objective_pop; pcc_rl_amd.objective; DESIGN.md
section 27): the numpy restatement of tests/models/reward_objective_model.py against the oracle's own reward column bit for bit,
zero weights skipping their column, the stated summation order (and that the test tells it from another valid order), every
refusal of the C ABI and of the Python side, the checkpoint's keys, and the compiler's resource report of the two kernels."""
import ctypes
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import reward_objective_model as model  # noqa: E402

import oracle  # noqa: E402
from pcc_rl_amd import native, objective  # noqa: E402
from pcc_rl_amd.native import lib  # noqa: E402
from pcc_rl_amd.objective import RewardObjective  # noqa: E402
from pcc_rl_amd.ppo import PPO, PopulationPPO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ_SYMBOLS = {"pcc_objective_scratch_doubles": 3, "pcc_reward_objective_pop": 9, "pcc_reward_objective": 8}


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def oracle_steps():
    """96 envs x 60 steps of the oracle under random actions: [T][N][19] float64."""
    B, T = 96, 60
    acts = np.random.default_rng(11).uniform(-1.0, 1.0, size=(B, T))
    ref = oracle.run_batch(acts, rng_mode=oracle.RNG_PHILOX, seed=3, want_obs=False)
    steps = np.ascontiguousarray(ref["steps"].reshape(B, T, model.STEP_COLS).transpose(1, 0, 2))
    assert steps.shape == (T, B, model.STEP_COLS)
    return steps


# ------------------------------------------------------------------------------------------------------------------ the model
def test_the_model_follows_the_registry():
    assert model.TERMS == objective.TERMS and model.N_TERMS == objective.N_TERMS
    assert [native.STEP_COLUMNS[c] for c in model.TERM_COLS] == list(objective.TERM_COLUMNS)
    assert native.STEP_COLUMNS[model.COL_REWARD] == "reward" and model.STEP_COLS == native.PCC_STEP_COLS
    assert objective.weight_row(RewardObjective.DEFAULT) == list(model.DEFAULT)
    text = open(os.path.join(ROOT, "include", "pcc_policy.h")).read()
    names = re.findall(r"\bPCC_OBJ_([A-Z_]+)\b\s*(?:= 0)?,", text[text.index("PCC_OBJ_THROUGHPUT = 0"):])[:model.N_TERMS]
    assert [n.lower() for n in names] == list(model.TERMS)       # the enum's order is the order of the names


def test_default_weights_are_the_oracle_reward_bit_for_bit(oracle_steps):
    steps = oracle_steps
    assert np.isfinite(steps[..., model.METRIC_COL0:]).all()
    _, acc, rew = model.terms(steps, model.DEFAULT)
    want = steps[..., model.COL_REWARD]
    assert np.array_equal(_u64(acc * model.REWARD_SCALE), _u64(want))
    assert np.array_equal(_u32(rew), _u32(want.astype(np.float32)))
    assert len(np.unique(want)) > steps.shape[0] * steps.shape[1] // 2      # (not a constant column)
    # as two members with the same weights, and through the names
    assert np.array_equal(_u32(model.reward(steps, [model.DEFAULT, model.DEFAULT], 2)), _u32(rew))
    assert np.array_equal(_u32(model.reward(steps, objective.weight_rows(None, 3), 3)), _u32(rew))


def test_a_zero_weight_skips_its_column(oracle_steps):
    steps = oracle_steps.copy()
    for c in (model.TERM_COLS[3], model.TERM_COLS[4], model.TERM_COLS[5]):
        steps[..., c] = np.nan                                    # the columns DEFAULT does not weigh
    tr, acc, rew = model.terms(steps, model.DEFAULT)
    assert np.isfinite(rew).all() and np.isfinite(acc).all() and not tr[3].any() and not tr[5].any()
    assert np.array_equal(_u32(rew), _u32(oracle_steps[..., model.COL_REWARD].astype(np.float32)))
    assert np.isnan(model.reward(steps, (10.0, -1e3, -2e3, 0.0, 1.0, 0.0))).all()      # weighed: it is read
    # the first included term starts the sum: -0.0 stays -0.0 (0.0 + -0.0 would be +0.0)
    one = np.zeros((1, 1, model.STEP_COLS))
    one[..., model.TERM_COLS[2]] = 0.0
    r = model.reward(one, (0.0, 0.0, -2e3, 0.0, 0.0, 0.0))
    assert _u32(r)[0, 0] == 0x80000000


def test_all_weights_zero_give_zero(oracle_steps):
    steps = oracle_steps.copy()
    steps[..., model.METRIC_COL0:] = np.nan
    tr, acc, rew = model.terms(steps, [0.0] * 6)
    assert not _u32(rew).any() and not tr.any()
    assert not _u64(model.sums(steps[:5], [0.0] * 6)).any()


def test_the_sums_follow_the_stated_order(oracle_steps):
    """kernel_order_sum against a loop written from the header's sentence, on shapes with a partial wavefront, a partial workgroup
    and more workgroups than one; and the check distinguishes the order: numpy's pairwise order over the same lane sums, also a
    valid one, differs in at least one bit on these inputs."""
    rng = np.random.default_rng(2)
    differs = 0
    for T, n_m in ((1, 1), (3, 63), (5, 65), (4, 257), (7, 700), (2, 256 * 300 + 5)):
        x = rng.random((T, n_m)) * 1e4
        lane = np.zeros(n_m)
        for t in range(T):
            lane = lane + x[t]
        G = -(-n_m // 256)
        padded = np.zeros(G * 256)
        padded[:n_m] = lane
        part = []
        for g in range(G):
            waves = []
            for v in range(4):
                w = padded[g * 256 + v * 64:g * 256 + v * 64 + 64].copy()
                d = 32
                while d >= 1:
                    for j in range(d):
                        w[j] = w[j] + w[j + d]
                    d //= 2
                waves.append(w[0])
            s = waves[0]
            for v in range(1, 4):
                s = s + waves[v]
            part.append(s)
        per = -(-G // 256)
        sub = np.zeros(256)
        for j in range(256):
            for g in range(j * per, min(j * per + per, G)):
                sub[j] = sub[j] + part[g]
        s = 128
        while s >= 1:
            for j in range(s):
                sub[j] = sub[j] + sub[j + s]
            s //= 2
        got = model.kernel_order_sum(x)
        assert _u64(got) == _u64(sub[0]), (T, n_m)
        other = model.pairwise_sum(x)
        assert abs(other - got) <= 1e-12 * abs(got)               # the same value ...
        differs += int(_u64(other).item() != _u64(got).item())         # ... in other bits
    assert differs >= 1
    steps = oracle_steps
    a, b = model.sums(steps, model.DEFAULT, 3), model.sums(steps, model.DEFAULT, 3, order=model.pairwise_sum)
    assert np.allclose(a, b, rtol=1e-12, atol=0.0) and not np.array_equal(_u64(a), _u64(b))
    assert not a[:, 3:6].any()                                    # a skipped term sums to 0
    _, _, rew = model.terms(steps, model.DEFAULT, 3)
    assert np.allclose(a[:, 6], rew.astype(np.float64).reshape(60, 3, 32).sum(axis=(0, 2)), rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_header_binding_and_library_agree():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcc_policy.h")).read(), flags=re.S)
    L = lib()
    for name, n_args in OBJ_SYMBOLS.items():
        m = re.search(r"\bint %s\s*\((.*?)\);" % name, text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, name
        assert name in native.SYMBOLS and hasattr(L, name)
        fn = getattr(L, name)
        assert len(fn.argtypes) == n_args and fn.restype is ctypes.c_int, name


def test_refusals_need_no_device():
    """Every -1 of the header, returned before any device call: the pointers here point nowhere."""
    L = lib()
    p = ctypes.c_void_p(4096)   # stands for a device pointer

    def pop(steps=p, T=4, N=12, K=3, weights=p, out=p, sums=p, scratch=p):
        return L.pcc_reward_objective_pop(steps, T, N, K, weights, out, sums, scratch, None)

    def alone(steps=p, T=4, N=12, weights=p, out=p, sums=p, scratch=p):
        return L.pcc_reward_objective(steps, T, N, weights, out, sums, scratch, None)

    for call in (pop, alone):
        for kw in ({"steps": None}, {"weights": None}, {"out": None}, {"scratch": None}, {"T": 0}, {"T": -1}, {"N": 0}, {"N": -12},
                   {"T": 1 << 30, "N": (1 << 40) * 3}):
            assert call(**kw) == -1, (call.__name__, kw)
    for kw in ({"K": 0}, {"K": -1}, {"K": 1025, "N": 2050}, {"N": 13}, {"K": 5}):
        assert pop(**kw) == -1, kw

    sd = L.pcc_objective_scratch_doubles
    for bad in ((0, 12, 3), (-1, 12, 3), (4, 0, 1), (4, -12, 3), (4, 12, 0), (4, 12, -1), (4, 2050, 1025), (4, 13, 3), (4, 12, 5),
                (1 << 30, (1 << 40) * 3, 3),
                (1, ((0x7fffffff // 7) + 1) * 256, 1)):           # more partials than an int holds
        assert sd(*bad) == -1, bad
    # the domain's edges
    assert sd(1, 1, 1) == 7 and sd(1, 256, 1) == 7 and sd(1, 257, 1) == 14 and sd(19, 3 * 331, 3) == 3 * 2 * 7
    assert sd(1, 1024, 1024) == 1024 * 7 and sd(1 << 20, 1024, 1024) == 1024 * 7
    assert sd(1, (0x7fffffff // 7) * 256, 1) == (0x7fffffff // 7) * 7


def test_kernels_use_no_scratch(tmp_path):
    """A build into a temporary file: both kernels are in the compiler's resource report with 0 bytes of scratch and no spilled
    register; the unit is one of its own, once; the older kernels keep the figures the suite pins."""
    from pcc_rl_amd import build as pbuild
    assert pbuild.UNITS.count("pcc_objective.hip") == 1
    out = str(tmp_path / "libpcc_sim_obj.so")
    pbuild.build_library(force=True, out=out)
    res = json.load(open(out + ".resources.json"))
    for name in ("objective_walk_kernel", "objective_merge_kernel"):
        assert name in res, name
        assert res[name]["scratch"] == 0 and res[name]["vgpr_spills"] == 0 and res[name]["sgpr_spills"] == 0, (name, res[name])
    assert sorted(n for n in res if n.startswith("objective_")) == ["objective_merge_kernel", "objective_walk_kernel"]
    assert sorted(n for n in res if n.startswith(("return_", "reward_"))) == ["return_merge_kernel", "return_walk_kernel", "reward_normalise_kernel"]
    assert sorted(n for n in res if n.startswith("episode_")) == ["episode_merge_kernel", "episode_walk_kernel"]
    assert (res["ppo_grad_mfma_kernel<30, 32, 16>"]["vgprs"], res["ppo_grad_mfma_kernel<30, 32, 16>"]["lds"]) == (256, 52736)
    assert res["policy_act_fixed_kernel<30, 32, 16>"]["vgprs"] == 87


# --------------------------------------------------------------------------------------------------------------- the Python side
class _Env(object):   # what the constructors' argument checks look at, without a simulator behind it
    obs_dim, device, n_senders, n_envs, max_steps = 30, "cuda:0", 1, 12, 400


class _CpuEnv(_Env):
    device = "cpu"


class _TwoSenders(_Env):
    n_senders = 2


def test_weights_are_parsed_and_refused():
    assert objective.weight_row({"latency": -5}) == [0.0, -5.0, 0.0, 0.0, 0.0, 0.0]            # a name left out weighs 0
    assert objective.weight_row((1, 2, 3, 4, 5, 6)) == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert objective.weight_rows({"loss": -1}, 2) == [[0.0, 0.0, -1.0, 0.0, 0.0, 0.0]] * 2
    assert objective.weight_rows([{"loss": -1}, (1, 0, 0, 0, 0, 0)], 2) == [[0.0, 0.0, -1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]]
    assert objective.weight_rows([1, 0, 0, 0, 0, 2], 6) == [[1.0, 0.0, 0.0, 0.0, 0.0, 2.0]] * 6  # six numbers: one row for all
    assert objective.parse("throughput=10,latency=-1000,loss=-2000") == {"throughput": 10.0, "latency": -1000.0, "loss": -2000.0}
    assert objective.parse("loss=-1;latency=-2e3") == [{"loss": -1.0}, {"latency": -2000.0}]
    for bad in ("loss", "loss=x"):
        with pytest.raises(ValueError, match="objective"):
            objective.parse(bad)
    with pytest.raises(ValueError, match="no term 'delay'"):
        objective.weight_row({"delay": 1.0})
    with pytest.raises(ValueError, match="5 weights"):
        objective.weight_row([1.0] * 5)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            objective.weight_row({"loss": bad})
        with pytest.raises(ValueError, match="finite"):
            objective.weight_row([1.0, bad, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="2 per-member objectives for 3 members"):
        objective.weight_rows([{"loss": -1}, {"loss": -2}], 3)
    with pytest.raises(ValueError, match="do not divide"):
        RewardObjective(12, 5, device="cpu")
    with pytest.raises(ValueError, match="no CPU path"):
        RewardObjective(12, 3, device="cpu")
    with pytest.raises(TypeError):
        RewardObjective.DEFAULT["loss"] = 0.0                      # the reference objective is read-only


def test_constructors_refuse():
    with pytest.raises(ValueError, match="objective=.*no CPU path"):
        PPO(_CpuEnv(), objective=RewardObjective.DEFAULT)
    with pytest.raises(ValueError, match="objective=.*one sender"):
        PPO(_TwoSenders(), objective=RewardObjective.DEFAULT)
    with pytest.raises(ValueError, match="no term 'delay'"):
        PPO(_Env(), objective={"delay": 1.0})
    with pytest.raises(ValueError, match="finite"):
        PPO(_Env(), objective={"loss": float("nan")})
    with pytest.raises(ValueError, match="2 per-member objectives for 1 members"):
        PPO(_Env(), objective=[{"loss": -1}, {"loss": -2}])
    with pytest.raises(ValueError, match="objective=.*no CPU path"):
        PopulationPPO(_CpuEnv(), 3, objective=RewardObjective.DEFAULT)
    with pytest.raises(ValueError, match="objective=.*one sender"):
        PopulationPPO(_TwoSenders(), 3, objective=RewardObjective.DEFAULT)
    with pytest.raises(ValueError, match="no term 'delay'"):
        PopulationPPO(_Env(), 3, objective={"delay": 1.0})
    with pytest.raises(ValueError, match="2 per-member objectives for 3 members"):
        PopulationPPO(_Env(), 3, objective=[{"loss": -1}, {"loss": -2}])
    with pytest.raises(ValueError, match="finite"):
        PopulationPPO(_Env(), 3, objective=[{"loss": -1}, {"loss": -2}, {"loss": float("inf")}])
    with pytest.raises(ValueError, match="BatchedNetworkEnv"):     # without the option: the argument checks as before
        PopulationPPO(_Env(), 3)


def _objective(rows):
    """A RewardObjective's host side alone."""
    o = RewardObjective.__new__(RewardObjective)
    o.n_envs, o.members, o.rows = 12, len(rows), [objective.weight_row(r) for r in rows]
    return o


def test_evolve_without_scores_refuses_mixed_objectives():
    pop = PopulationPPO.__new__(PopulationPPO)
    pop.env, pop.members, pop.track_episodes = _Env(), 2, True
    pop.objective = _objective([{"loss": -1}, {"latency": -1}])
    assert not pop.objective.uniform()
    with pytest.raises(ValueError, match="different objectives do not rank"):
        pop.evolve()
    pop.objective = _objective([{"loss": -1}, {"loss": -1}])
    assert pop.objective.uniform()
    pop.ledger = types.SimpleNamespace(scores=lambda: (_ for _ in ()).throw(KeyError("the ledger is asked")))
    with pytest.raises(KeyError, match="the ledger is asked"):     # one objective for all: the check passes, the ledger is read
        pop.evolve()


def test_the_checkpoint_records_the_option():
    """_common_state / _restore on a PPO object with their fields and nothing else: no device, no library."""
    class _Snap(_CpuEnv):
        restored = None

        def snapshot(self):
            return "snapshot"

        def restore(self, s):
            self.restored = s

    class _Obj(object):
        loaded = None

        def state_dict(self):
            return {"weights": "w"}

        def load_state_dict(self, sd):
            self.loaded = sd

    def trainer(on):
        t = PPO.__new__(PPO)
        t.env, t.obs, t.rng, t.iteration, t.streams, t.target_kl = _Snap(), torch.zeros(12, 30), "torch", 0, None, None
        t.normalize_obs = t.track_episodes = t.normalize_reward = t.diagnostics = False
        if on:
            t.objective = _Obj()
        t._load_params = lambda sd: None
        return t

    on, off = trainer(True)._common_state(), trainer(False)._common_state()
    assert on["objective"] is True and set(on) - set(off) == {"objective", "objective_state"}     # without the option: the keys of before
    assert set(off) == {"obs", "torch_rng", "device_rng", "env"}
    b = trainer(True)
    b._restore(on)
    assert b.env.restored == "snapshot" and b.objective.loaded == {"weights": "w"}
    for mine, theirs in ((False, on), (True, off)):
        other = trainer(mine)
        with pytest.raises(ValueError, match="written with objective="):
            other._restore(theirs)
        assert other.env.restored is None      # refused before anything is restored
