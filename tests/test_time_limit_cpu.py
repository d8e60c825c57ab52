"""Time-limit bootstrapping, the part that needs no GPU (include/pcc_policy.h: pcc_terminal_obs, pcc_gae_boot, pcc_gae_boot_pop;
pcc_rl_amd.timelimit): the numpy restatement of tests/models/time_limit_model.py against ppo.gae and a
hand-computed case, ppo.gae(term_value=...) against the restatement, the slot bound, every refusal of the host side, the three
symbols, the compiler's resource report of the two kernels, and what the constructors refuse."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import time_limit_model as model  # noqa: E402

from pcc_rl_amd import native, timelimit  # noqa: E402
from pcc_rl_amd.metrics import METRIC_NAMES, metric_info  # noqa: E402
from pcc_rl_amd.native import lib  # noqa: E402
from pcc_rl_amd.ppo import PPO, PopulationPPO, gae  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TL_SYMBOLS = {"pcc_terminal_obs": 13, "pcc_gae_boot": 14, "pcc_gae_boot_pop": 14}
GAMMA, LAM = 0.99, 0.95   # (the trainers' defaults.  ppo.gae multiplies by float32(gamma * lam), the kernels by float32(gamma) *
#                            float32(lam): for these two the products are the same float32, which the first test asserts)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _rows(T, N, seed, p_done=0.0):
    rng = np.random.default_rng(seed)
    rew = rng.standard_normal((T, N)).astype(np.float32)
    val = rng.standard_normal((T, N)).astype(np.float32) * 3
    last = rng.standard_normal(N).astype(np.float32)
    done = (rng.random((T, N)) < p_done).astype(np.uint8)
    return rew, val, done, last


# ---------------------------------------------------------------------------------------------------------- the model alone
def test_without_a_done_the_model_is_ppo_gae():
    assert np.float32(GAMMA) * np.float32(LAM) == np.float32(GAMMA * LAM)
    for T, N in ((1, 1), (17, 5), (64, 3)):
        rew, val, done, last = _rows(T, N, T + N)
        n_slots = 2
        tv, tc = np.full((n_slots, N), 1e6, dtype=np.float32), np.zeros(N, dtype=np.int32)   # (never read)
        adv, ret = model.gae_boot(rew, val, done, last, tv, tc, GAMMA, LAM)
        want_adv, want_ret = gae(torch.from_numpy(rew), torch.from_numpy(val), torch.from_numpy(done), torch.from_numpy(last), GAMMA, LAM)
        assert np.array_equal(_bits(adv), _bits(want_adv.numpy())) and np.array_equal(_bits(ret), _bits(want_ret.numpy())), (T, N)
        plain_adv, plain_ret = model.gae_boot(rew, val, done, last, None, None, GAMMA, LAM)    # pcc_gae's restatement
        assert np.array_equal(_bits(adv), _bits(plain_adv)) and np.array_equal(_bits(ret), _bits(plain_ret))


def test_three_steps_by_hand():
    """gamma = lam = 0.5, one env, a done after the second step, exactly representable numbers.
    t = 2: delta = 1 + 0.5 * 8 - 2 = 3, adv = 3.   t = 1 (done; v_term = 4): delta = 2 + 0.5 * 4 - 6 = -2, adv = -2: the recursion is
    cut.  t = 0: delta = 4 + 0.5 * 6 - 2 = 5, adv = 5 + 0.25 * -2 = 4.5."""
    rew = np.array([[4.0], [2.0], [1.0]], dtype=np.float32)
    val = np.array([[2.0], [6.0], [2.0]], dtype=np.float32)
    done = np.array([[0], [1], [0]], dtype=np.uint8)
    last = np.array([8.0], dtype=np.float32)
    adv, ret = model.gae_boot(rew, val, done, last, np.array([[4.0]], dtype=np.float32), np.array([1], dtype=np.int32), 0.5, 0.5)
    assert adv[:, 0].tolist() == [4.5, -2.0, 3.0] and ret[:, 0].tolist() == [6.5, 4.0, 5.0]
    adv0, _ = model.gae_boot(rew, val, done, last, None, None, 0.5, 0.5)       # without the bootstrap: delta(1) = 2 - 6 = -4
    assert adv0[:, 0].tolist() == [4.0, -4.0, 3.0]
    # a done whose slot is not stored (n_slots = 1, it is the env's second) is pcc_gae's
    done2 = np.array([[1], [1], [0]], dtype=np.uint8)
    adv2, _ = model.gae_boot(rew, val, done2, last, np.array([[4.0]], dtype=np.float32), np.array([2], dtype=np.int32), 0.5, 0.5)
    assert adv2[:, 0].tolist() == [4.0 + 0.5 * 4.0 - 2.0, -4.0, 3.0]           # row 0: slot 0 = 4; row 1: slot 1 >= n_slots


def test_ppo_gae_with_terminal_values_is_the_model():
    for T, N, n_slots, p in ((1, 1, 1, 1.0), (17, 9, 3, 0.2), (64, 4, 2, 0.1), (12, 6, 1, 0.5)):
        rew, val, done, last = _rows(T, N, 7 * T + N, p)
        if T > 2:
            done[1, 0] = done[2, 0] = 1                                        # two in adjacent rows
        rng = np.random.default_rng(T)
        tv = rng.standard_normal((n_slots, N)).astype(np.float32)
        tc = done.sum(0).astype(np.int32)
        assert T < 12 or (tc > n_slots).any()                                  # a count above n_slots is among them
        want_adv, want_ret = model.gae_boot(rew, val, done, last, tv, tc, GAMMA, LAM)
        adv, ret = gae(torch.from_numpy(rew), torch.from_numpy(val), torch.from_numpy(done), torch.from_numpy(last), GAMMA, LAM,
                       term_value=torch.from_numpy(tv), term_count=torch.from_numpy(tc))
        assert np.array_equal(_bits(adv.numpy()), _bits(want_adv)) and np.array_equal(_bits(ret.numpy()), _bits(want_ret)), (T, N)
        plain, _ = gae(torch.from_numpy(rew), torch.from_numpy(val), torch.from_numpy(done), torch.from_numpy(last), GAMMA, LAM)
        assert not np.array_equal(plain.numpy(), want_adv)
    with pytest.raises(ValueError, match="term_count"):
        gae(torch.zeros(2, 2), torch.zeros(2, 2), torch.zeros(2, 2), torch.zeros(2), term_value=torch.zeros(1, 2))


def test_terminal_row_model():
    """Slicing, the float64 division and its one cast, slots, zero rows and counts."""
    F, H = 2, 3
    cols, scales = model.feature_columns([1, 11])                              # recv rate (1e7) and send ratio (1)
    assert (cols, scales) == ([8, 18], [1e7, 1.0])
    obs = np.arange(2 * 2 * H * F, dtype=np.float32).reshape(2, 2, H * F)
    steps = np.zeros((2, 2, model.STEP_COLS))
    steps[..., 8], steps[..., 18] = 3333333.3, 1.0 / 3.0
    done = np.array([[0, 1], [1, 1]], dtype=np.uint8)
    term, count = model.terminal_obs(obs, steps, done, F, cols, scales, 1)
    assert count.tolist() == [1, 2] and term.shape == (1, 2, 6) and term.dtype == np.float32
    new = [np.float32(3333333.3 / 1e7), np.float32(1.0 / 3.0)]
    assert term[0, 0].tolist() == obs[1, 0, F:].tolist() + new                 # env 0: its done is in row 1
    assert term[0, 1].tolist() == obs[0, 1, F:].tolist() + new                 # env 1: the first of its two; the second is not stored
    assert new[0] != np.float32(np.float32(3333333.3) / np.float32(1e7))     # (the division is float64's)
    term2, _ = model.terminal_obs(obs, steps, done, F, cols, scales, 2)
    assert not term2[1, 0].any() and term2[1, 1].tolist() == obs[1, 1, F:].tolist() + new


def test_feature_columns_follow_the_registry():
    class _E(object):
        feature_ids = list(range(len(METRIC_NAMES)))

    cols, scales = timelimit.feature_columns(_E())
    assert (cols, scales) == model.feature_columns(_E.feature_ids)
    assert [native.STEP_COLUMNS[c] for c in cols] == METRIC_NAMES
    assert scales == [metric_info(n)[2] for n in METRIC_NAMES]
    L = lib()
    for i, s in enumerate(scales):                                             # ... and pcc_metric_info's
        sc = ctypes.c_double()
        assert L.pcc_metric_info(i, None, None, ctypes.byref(sc)) == 0 and sc.value == s


# ---------------------------------------------------------------------------------------------------------- the slot bound
def test_no_env_exceeds_the_slots():
    """Two dones of an env are at least max_steps rows apart, whatever masked resets come between: ceil(T / max_steps) slots hold
    every done of T rows."""
    rng = np.random.default_rng(5)
    seen_full = False
    for _ in range(2000):
        T, max_steps = int(rng.integers(1, 70)), int(rng.integers(1, 12))
        first = int(rng.integers(0, max_steps))
        resets = set(int(t) for t in rng.integers(0, T, size=int(rng.integers(0, 4))))
        times = model.done_times(T, max_steps, first, resets)
        assert all(b - a >= max_steps for a, b in zip(times, times[1:])), (T, max_steps, first, resets)
        assert len(times) <= model.slots(T, max_steps) == timelimit.slots(T, max_steps), (T, max_steps, first, resets)
        seen_full |= len(times) == model.slots(T, max_steps) > 1
    assert seen_full                                                           # the bound is reached
    assert [timelimit.slots(*a) for a in ((1, 400), (400, 400), (401, 400), (64, 8), (12, 8), (17, 5))] == [1, 1, 2, 8, 2, 4]
    with pytest.raises(ValueError):
        timelimit.slots(0, 400)


# ------------------------------------------------------------------------------------------------------------ the library
def test_header_binding_and_library_agree():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcc_policy.h")).read(), flags=re.S)
    L = lib()
    for name, n_args in TL_SYMBOLS.items():
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
    i32s = lambda v: (ctypes.c_int32 * len(v))(*v)
    dbls = lambda v: (ctypes.c_double * len(v))(*v)
    inf, nan = float("inf"), float("nan")

    def term(obs=p, steps=p, done=p, T=4, N=12, H=10, F=3, cols=(14, 17, 18), scales=(1.0, 1.0, 1.0), n_slots=1, out=p, count=p):
        return L.pcc_terminal_obs(obs, steps, done, T, N, H, F, None if cols is None else i32s(cols),
                                  None if scales is None else dbls(scales), n_slots, out, count, None)

    for kw in ({"obs": None}, {"steps": None}, {"done": None}, {"cols": None}, {"scales": None}, {"out": None}, {"count": None},
               {"T": 0}, {"T": -1}, {"N": 0}, {"N": -12}, {"n_slots": 0}, {"n_slots": -1}, {"H": 0}, {"H": -1}, {"F": 0}, {"F": -1},
               {"F": 17, "cols": (7,) * 17, "scales": (1.0,) * 17}, {"cols": (14, 19, 18)}, {"cols": (-1, 17, 18)}, {"cols": (14, 17, 1 << 20)},
               {"scales": (1.0, 0.0, 1.0)}, {"scales": (1.0, -1e7, 1.0)}, {"scales": (inf, 1.0, 1.0)}, {"scales": (1.0, 1.0, nan)},
               {"scales": (1.0, -inf, 1.0)}):
        assert term(**kw) == -1, kw

    def boot(rew=p, val=p, done=p, last=p, tv=p, tc=p, n_slots=1, T=4, N=12, adv=p, ret=p):
        return L.pcc_gae_boot(rew, val, done, last, tv, tc, n_slots, T, N, 0.99, 0.95, adv, ret, None)

    def boot_pop(rew=p, val=p, done=p, last=p, tv=p, tc=p, n_slots=1, T=4, N=12, K=3, hyper=p, adv=p, ret=p):
        return L.pcc_gae_boot_pop(rew, val, done, last, tv, tc, n_slots, T, N, K, hyper, adv, ret, None)

    for call in (boot, boot_pop):
        for kw in ({"rew": None}, {"val": None}, {"done": None}, {"last": None}, {"tv": None}, {"tc": None}, {"adv": None}, {"ret": None},
                   {"T": 0}, {"T": -3}, {"N": 0}, {"N": -12}, {"n_slots": 0}, {"n_slots": -2}):
            assert call(**kw) == -1, (call.__name__, kw)
    for kw in ({"hyper": None}, {"K": 0}, {"K": -1}, {"K": 1025, "N": 2050}, {"N": 13}, {"K": 5}):
        assert boot_pop(**kw) == -1, kw


def test_kernels_use_no_scratch(tmp_path):
    """A build into a temporary file: the two kernels are in the compiler's resource report with 0 bytes of scratch, no spilled
    register and no LDS; the unit is one of its own, and the figures tests/test_population_cpu.py pins for the policy kernels are
    still what the report says."""
    from pcc_rl_amd import build as pbuild
    assert "pcc_timelimit.hip" in pbuild.UNITS
    out = str(tmp_path / "libpcc_sim_tl.so")
    pbuild.build_library(force=True, out=out)
    res = json.load(open(out + ".resources.json"))
    for name in ("terminal_obs_kernel", "gaeboot_kernel"):
        assert name in res, name
        assert res[name]["scratch"] == 0 and res[name]["vgpr_spills"] == 0 and res[name]["sgpr_spills"] == 0, (name, res[name])
        assert res[name]["lds"] == 0, (name, res[name])
    assert sorted(n for n in res if "terminal_" in n or "gaeboot" in n) == ["gaeboot_kernel", "terminal_obs_kernel"]
    assert "gae_kernel" in res
    assert (res["ppo_grad_mfma_kernel<30, 32, 16>"]["vgprs"], res["ppo_grad_mfma_kernel<30, 32, 16>"]["lds"]) == (256, 52736)
    assert res["policy_act_fixed_kernel<30, 32, 16>"]["vgprs"] == 87


# ------------------------------------------------------------------------------------------------------------ constructors
class _Env(object):   # what the constructors' argument checks look at, without a simulator behind it
    obs_dim, device, n_senders, n_envs, max_steps = 30, "cuda:0", 1, 12, 400


class _CpuEnv(_Env):
    device = "cpu"


class _TwoSenders(_Env):
    n_senders = 2


def test_constructors_refuse():
    with pytest.raises(ValueError, match="bootstrap_time_limit=True.*no CPU path"):
        PPO(_CpuEnv(), bootstrap_time_limit=True)
    with pytest.raises(ValueError, match="bootstrap_time_limit=True.*one sender"):
        PPO(_TwoSenders(), bootstrap_time_limit=True)
    with pytest.raises(ValueError, match="no CPU path"):
        timelimit.TimeLimitBootstrap(_CpuEnv(), 64)
    with pytest.raises(ValueError, match="one sender"):
        timelimit.TimeLimitBootstrap(_TwoSenders(), 64)
    with pytest.raises(ValueError, match="BatchedNetworkEnv"):   # the argument checks as before
        PopulationPPO(_Env(), 3, bootstrap_time_limit=True)
    with pytest.raises(ValueError, match="one sender"):
        timelimit.terminal_observations(_TwoSenders(), None, None, None)


def test_the_checkpoint_records_the_option():
    """_common_state / _restore on a PPO object with their fields and nothing else: no device, no library."""
    class _Snap(_CpuEnv):
        restored = None

        def snapshot(self):
            return "snapshot"

        def restore(self, s):
            self.restored = s

    def trainer(on):
        t = PPO.__new__(PPO)
        t.env, t.obs, t.rng, t.iteration, t.streams, t.target_kl = _Snap(), torch.zeros(12, 30), "torch", 0, None, None
        t.normalize_obs = t.track_episodes = t.normalize_reward = t.diagnostics = False
        t.bootstrap_time_limit = on
        t._load_params = lambda sd: None
        return t

    on, off = trainer(True)._common_state(), trainer(False)._common_state()
    assert on["bootstrap_time_limit"] is True and set(on) - set(off) == {"bootstrap_time_limit"}   # the option, no state; the keys of before
    b = trainer(True)
    b._restore(on)
    assert b.env.restored == "snapshot"
    for mine, theirs in ((False, on), (True, off)):
        other = trainer(mine)
        with pytest.raises(ValueError, match="written with bootstrap_time_limit="):
            other._restore(theirs)
        assert other.env.restored is None      # refused before anything is restored
