"""Update diagnostics and the KL guard on the GPU (include/pcc_policy.h: pcc_policy_act_rows_pop, pcc_update_diag_pop and its
stand-alone form; pcc_rl_amd.updiag.UpdateDiagnostics; PPO / PopulationPPO with diagnostics=True / target_kl).

The rows of diag are held against tests/models/update_diag_model.py: count, the clipped count and nonfinite exactly (every case keeps
its clip margin: tests/test_update_diag_cpu.py), approx_kl, the variances and explained_variance within the model's bounds --
per sample delta_i = 13 x 2^-24 (z_i^2 / 2 + |log_std| + 1 + |logp_old_i|) for the float32 log-ratio, mean(|expm1(d_i)| delta_i +
delta_i^2) + 8 n 2^-53 max k for the KL, moment_bounds of section 19 for the variances -- and max_abs_log_ratio within the largest
delta.  Everything else is exact: the decision and hyper_live against the rule applied to the device's own approx_kl, a member
against the stand-alone call on a copy of its columns, a repeated call, the padding, pcc_policy_act_rows_pop against
pcc_policy_act_pop row by row, and the trainers' parameters against runs without the options."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import update_diag_model as model  # noqa: E402

import pcc_rl_amd  # noqa: E402
from pcc_rl_amd.native import lib  # noqa: E402
from pcc_rl_amd.ppo import PPO, PopulationPPO, population_permutations  # noqa: E402

DEV = "cuda:0"
CASES = sorted(model.CASES)
PAD, POISON = 3, -7777.25            # doubles behind every diag row, and what they hold
STRIDE, INDEX = 128, 70              # a parameter block of 128 floats with log_std at 70
_p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case's inputs (numpy, and on the device) and every member's reference row and bounds: computed once, never changed."""
    case = model.make_case(name)
    refs = [model.member_reference(case, m) for m in range(case["K"])]
    dev = {k: torch.from_numpy(case[k]).to(DEV) for k in ("act", "logp_old", "mean_new", "ret", "val")}
    return case, refs, dev


def _params(log_std):
    p = torch.full((len(log_std), STRIDE), 55.5, device=DEV)   # (what must not be read as log_std)
    p[:, INDEX] = torch.as_tensor(np.asarray(log_std, dtype=np.float32)).to(DEV)
    return p


def _hyper(K, clip):
    h = np.full((K, 8), 7.5, dtype=np.float32)
    h[:, 0] = 1e-3 * (1 + np.arange(K))
    h[:, 1] = clip
    return torch.from_numpy(h).to(DEV)


def _diag(case, dev, kl_limit=0.0, epoch=1, stop=None, decide=True, mean_new=None, hyper=None):
    """pcc_update_diag_pop on the device rows; returns (diag with its poisoned padding, stop, hyper_live)."""
    T, N, K, step = case["T"], case["N"], case["K"], case["row_step"]
    need = lib().pcc_update_diag_scratch_doubles(T, step, N, K)
    assert need > 0
    scratch = torch.full((need,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((K, 8 + PAD), POISON, dtype=torch.float64, device=DEV)
    hyper = _hyper(K, case["clip"]) if hyper is None else hyper
    if decide:
        stop = torch.zeros(K, dtype=torch.int32, device=DEV) if stop is None else stop
        live = torch.full((K, 8), -3.25, device=DEV)
    else:
        stop = live = None
    rc = lib().pcc_update_diag_pop(_p(dev["act"]), _p(dev["logp_old"]), _p(dev["mean_new"] if mean_new is None else mean_new), _p(dev["ret"]),
                                   _p(dev["val"]), T, step, N, K, _p(_params(case["log_std"])), STRIDE, INDEX, _p(hyper), float(kl_limit),
                                   epoch, _p(out), out.stride(0), _p(stop), _p(live), _p(scratch), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out, stop, live


def _check_row(row, ref, b, what, used):
    """One member's device row against its reference and bounds; `used` collects the largest fraction of each bound used."""
    assert row[0] == ref["count"] and row[7] == ref["nonfinite"], (what, row, ref)
    assert row[2] == ref["clipped"] / ref["count"], (what, row[2], ref["clipped"])   # (one IEEE division of two exact counts)
    for col, name in ((1, "approx_kl"), (5, "var_ret"), (6, "var_resid"), (3, "explained_variance"), (4, "max_abs_log_ratio")):
        err = abs(row[col] - ref[name])
        print("%s %s: device %.17g reference %.17g error %.3g bound %.3g" % (what, name, row[col], ref[name], err, b[name]))
    for col, name in ((1, "approx_kl"), (5, "var_ret"), (6, "var_resid"), (3, "explained_variance"), (4, "max_abs_log_ratio")):
        if np.isnan(ref[name]):
            assert np.isnan(row[col]), (what, name, row[col])
            continue
        err = abs(row[col] - ref[name])
        assert err <= b[name], (what, name, row[col], ref[name], err, b[name])
        if b[name] > 0.0:
            used[name] = max(used.get(name, 0.0), err / b[name])
    assert row[1] >= 0.0 and row[5] >= 0.0 and row[6] >= 0.0


# ------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_rows_against_the_model(name):
    case, refs, dev = _case(name)
    out, stop, live = _diag(case, dev)
    rows = out.cpu().numpy()
    used = {}
    for m in range(case["K"]):
        _check_row(rows[m, :8], refs[m][0], refs[m][1], "%s member %d" % (name, m), used)
    print("%s: largest fraction of each bound used: %s" % (name, {k: "%.3g" % v for k, v in sorted(used.items())}))
    assert (rows[:, 8:] == POISON).all()                       # the padding is never written
    assert not stop.any() and torch.equal(_bits(live), _bits(_hyper(case["K"], case["clip"])))   # no limit: nobody stops
    again, _, _ = _diag(case, dev)                             # the same inputs give the same bits
    assert torch.equal(_bits(again), _bits(out))
    alone, _, _ = _diag(case, dev, decide=False)               # ... with or without the decision
    assert torch.equal(_bits(alone), _bits(out))


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_members_equal_stand_alone_calls(name):
    case, _, dev = _case(name)
    out, _, _ = _diag(case, dev)
    T, n_m, step = case["T"], case["n_m"], case["row_step"]
    scratch = torch.full((lib().pcc_update_diag_scratch_doubles(T, step, n_m, 1),), float("nan"), dtype=torch.float64, device=DEV)
    for m in range(case["K"]):
        cols = [dev[k][:, m * n_m:(m + 1) * n_m].contiguous() for k in ("act", "logp_old", "mean_new", "ret", "val")]
        params = torch.full((INDEX + 1,), 55.5, device=DEV)
        params[INDEX] = float(case["log_std"][m])
        row = torch.full((8,), POISON, dtype=torch.float64, device=DEV)
        assert lib().pcc_update_diag(*[_p(c) for c in cols], T, step, n_m, _p(params), INDEX, case["clip"], _p(row), _p(scratch), _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(row), _bits(out[m, :8])), (name, m, row.tolist(), out[m, :8].tolist())


@pytest.mark.gpu
def test_a_nan_mean_stops_its_member_alone():
    case, refs, dev = _case("three-members")
    clean, _, _ = _diag(case, dev, kl_limit=1e9)
    bad = dev["mean_new"].clone()
    bad[2, case["n_m"] + 5] = float("nan")                     # one sample of member 1
    out, stop, live = _diag(case, dev, kl_limit=1e9, epoch=3, mean_new=bad)
    assert torch.isnan(out[1, 1]) and out[1, 7] == 1.0 and out[1, 0] == refs[1][0]["count"]
    assert 0.0 < float(out[1, 4]) <= float(clean[1, 4])          # the NaN does not enter the maximum
    assert stop.tolist() == [0, 3, 0]
    hyper = _hyper(3, case["clip"])
    assert live[1, 0] == 0.0 and torch.equal(_bits(live[1, 1:]), _bits(hyper[1, 1:]))
    for m in (0, 2):                                           # the others: the bits of the run without the NaN
        assert torch.equal(_bits(out[m]), _bits(clean[m])) and torch.equal(_bits(live[m]), _bits(hyper[m])), m
    for limit in (0.0, -1.0):                                  # diagnostics only: even a NaN does not stop
        _, stop, live = _diag(case, dev, kl_limit=limit, mean_new=bad)
        assert stop.tolist() == [0, 0, 0] and torch.equal(_bits(live), _bits(hyper))


def _limit_between(kls, bnds, lo_member, hi_member):
    """A limit between two members' reference KLs, further from each than its bound."""
    lo, hi = kls[lo_member], kls[hi_member]
    limit = float(np.sqrt(lo * hi))
    assert lo + bnds[lo_member] < limit < hi - bnds[hi_member]
    return limit


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["three-members", "four-members", "step-past-T"])
def test_the_decision_and_hyper_live(name):
    """The limits lie further from every member's reference KL than its bound, so the reference and the device agree on who stops;
    stop and hyper_live are held, exactly, against the rule applied to the device's own approx_kl.  stop is sticky."""
    case, refs, dev = _case(name)
    K = case["K"]
    kls, bnds = [r[0]["approx_kl"] for r in refs], [r[1]["approx_kl"] for r in refs]
    order = np.argsort(kls)
    hyper = _hyper(K, case["clip"]).cpu().numpy()
    # epoch 2: a limit between the two largest KLs stops the largest alone
    first = _limit_between(kls, bnds, order[-2], order[-1])
    out, stop, live = _diag(case, dev, kl_limit=first, epoch=2)
    want_stop, want_live = model.decide(np.zeros(K), out[:, 1].cpu().numpy(), first, 2, hyper)
    assert want_stop.tolist() == [2 if m == order[-1] else 0 for m in range(K)]
    assert np.array_equal(model.decide(np.zeros(K), np.array(kls), first, 2, hyper)[0], want_stop)   # the reference agrees
    assert stop.cpu().numpy().tolist() == want_stop.tolist()
    assert torch.equal(_bits(live), _bits(torch.from_numpy(want_live).to(DEV)))
    # epoch 3, the same stop: a limit between the two smallest stops all but the smallest; the first keeps its 2
    second = _limit_between(kls, bnds, order[0], order[1])
    out2, stop2, live2 = _diag(case, dev, kl_limit=second, epoch=3, stop=stop)
    want_stop2, want_live2 = model.decide(want_stop, out2[:, 1].cpu().numpy(), second, 3, hyper)
    assert sorted(want_stop2.tolist()) == sorted([0, 2] + [3] * (K - 2))
    assert stop2.cpu().numpy().tolist() == want_stop2.tolist()
    assert torch.equal(_bits(live2), _bits(torch.from_numpy(want_live2).to(DEV)))
    assert torch.equal(_bits(out2), _bits(out))                # the decision does not touch the rows
    # epoch 4 with a limit nobody exceeds: what stopped stays stopped
    _, stop3, live3 = _diag(case, dev, kl_limit=1e9, epoch=4, stop=stop2)
    assert stop3.cpu().numpy().tolist() == want_stop2.tolist() and torch.equal(_bits(live3), _bits(live2))
    for limit in (0.0, -5.0):                                  # never stops
        _, s, l = _diag(case, dev, kl_limit=limit, epoch=1)
        assert not s.any() and torch.equal(_bits(l), _bits(torch.from_numpy(hyper).to(DEV)))


ACT_SHAPES = [(30, 32, 16, 3, 257, 5, 1), (30, 32, 16, 3, 257, 5, 2), (30, 32, 16, 1, 300, 4, 9), (30, 32, 16, 1, 300, 4, 1),
              (12, 20, 10, 1, 130, 3, 1), (21, 24, 12, 2, 131, 5, 2), (21, 24, 12, 1, 70, 3, 1), (21, 24, 12, 1, 70, 3, 2),
              (21, 24, 12, 1, 4133, 5, 1), (100, 64, 48, 1, 77, 3, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ACT_SHAPES, ids=lambda s: "-".join(str(x) for x in s))
def test_act_rows_equal_row_by_row_calls(shape):
    """(D, h1, h2, K, n_m, T, row_step): the reference's --arch at 30 observations (the fully unrolled kernel), another --arch at a
    length of that table (the generic kernel) and a shape of the tiled kernel; one member with every row selected is ONE launch over
    all rows, anything else a launch per row.  In the one-launch cases no row ends on a tile (32 rows) or workgroup edge -- 300 envs
    against the fixed kernel's 256; 70, 77 and 4133 against the tiled kernel's tiles, the last with 646 tiles over 128 workgroups that
    each walk several -- so a row's envs share tiles and workgroups with the next row's.  The selected rows carry pcc_policy_act_pop's bits, every other row is as it was."""
    D, h1, h2, K, n_m, T, step = shape
    N = K * n_m
    g = torch.Generator(device=DEV).manual_seed(D + T)
    n_params = 2 * (h1 * D + h1 + h2 * h1 + 2 * h2 + 1) + 1
    stride = (n_params + 63) // 64 * 64
    params = 0.3 * torch.randn((K, stride), device=DEV, generator=g)
    obs = torch.randn((T, N, D), device=DEV, generator=g)
    L = lib()
    want_mean, want_val = torch.full((T, N), POISON, device=DEV), torch.full((T, N), POISON, device=DEV)
    for t in range(0, T, step):
        assert L.pcc_policy_act_pop(_p(obs[t]), N, D, _p(params), stride, K, h1, h2, None, _p(want_mean[t]), None, None, _p(want_val[t]),
                                    _stream()) == 0
    for with_mean, with_val in ((True, True), (True, False), (False, True)):
        mean, val = torch.full((T, N), POISON, device=DEV), torch.full((T, N), POISON, device=DEV)
        assert L.pcc_policy_act_rows_pop(_p(obs), T, step, N, D, _p(params), stride, K, h1, h2, _p(mean) if with_mean else None,
                                         _p(val) if with_val else None, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(mean), _bits(want_mean if with_mean else torch.full_like(mean, POISON))), (shape, with_mean, with_val)
        assert torch.equal(_bits(val), _bits(want_val if with_val else torch.full_like(val, POISON))), (shape, with_mean, with_val)
    rows = list(range(0, T, step))
    assert torch.isfinite(want_mean[rows]).all() and (want_mean[rows] != POISON).all()
    others = [t for t in range(T) if t not in rows]
    assert (want_mean[others] == POISON).all() and (want_val[others] == POISON).all()


# ------------------------------------------------------------------------------------------------------------ the trainers
POOLS = (2, 8, 32)   # (fixed ring pools: the library's default depends on the free device memory, and a snapshot needs equal pools)
K, N_M, T = 3, 512, 12
LRS = [1e-4, 0.3, 1e-4]   # member 1 runs away
TARGET = 0.05
NEW_KEYS = ["approx_kl", "clip_fraction", "epochs_run", "explained_variance", "max_log_ratio", "nonfinite"]


def _env(n, seed, **kw):
    return pcc_rl_amd.BatchedNetworkEnv(n, device=DEV, seed=seed, ring_pools=POOLS, **kw)


@functools.lru_cache(maxsize=None)
def _population_run(diagnostics, target_kl, epochs, diag_rows=None):
    """One collect() and one update() of 3 members x 512 envs x 12 steps from the same env seed, policies, noise and permutations."""
    env = _env(K * N_M, 41)
    pop = PopulationPPO(env, K, horizon=T, lr=LRS, seeds=[4, 5, 6], epochs=epochs, diagnostics=diagnostics, target_kl=target_kl,
                        diag_rows=diag_rows)
    noise = torch.randn((T, K * N_M), device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    g = torch.Generator().manual_seed(9)
    perms = [population_permutations(T, K * N_M, K, generator=g).to(DEV) for _ in range(4)]
    stats = pop.update(*pop.collect(noise=noise)[:5], perms=perms)
    torch.cuda.synchronize()
    out = {"flat": pop.flat.clone(), "adam_m": pop.adam_m.clone(), "adam_v": pop.adam_v.clone(), "adam_t": pop.adam_t, "stats": stats,
           "hyper": pop.hyper.clone(), "live": None if pop.diag is None else pop.diag.hyper_live.clone(),
           "row_step": None if pop.diag is None else pop.diag.row_step}
    env.close()
    return out


@pytest.mark.gpu
def test_diagnostics_alone_change_no_parameter():
    off, on = _population_run(False, None, 4), _population_run(True, None, 4)
    for name in ("flat", "adam_m", "adam_v"):
        assert torch.equal(_bits(on[name]), _bits(off[name])), name
    assert on["adam_t"] == off["adam_t"] == 12
    assert sorted(off["stats"]) == ["clip_frac", "entropy", "pg", "vf"]                    # the keys of before
    assert sorted(set(on["stats"]) - set(off["stats"])) == NEW_KEYS
    for k in off["stats"]:
        assert on["stats"][k] == off["stats"][k], k
    s = on["stats"]
    assert s["epochs_run"] == [4, 4, 4] and s["nonfinite"][0] == 0 and s["nonfinite"][2] == 0
    assert all(len(s[k]) == K for k in NEW_KEYS)
    assert s["approx_kl"][0] >= 0.0 and not (s["approx_kl"][1] <= s["approx_kl"][0]), s
    assert all(0.0 <= c <= 1.0 for c in s["clip_fraction"]), s
    assert s["explained_variance"][0] <= 1.0 and s["max_log_ratio"][0] >= 0.0
    assert torch.equal(on["live"], on["hyper"])                                            # nobody was stopped
    sub = _population_run(True, None, 4, 4)                                                # diag_rows=4 of 12: every third row
    assert sub["row_step"] == 3 and torch.equal(_bits(sub["flat"]), _bits(off["flat"]))
    assert sub["stats"]["approx_kl"] != s["approx_kl"]


@pytest.mark.gpu
def test_the_kl_guard_stops_the_runaway_member_alone():
    off, guarded, one = _population_run(False, None, 4), _population_run(False, TARGET, 4), _population_run(False, TARGET, 1)
    s = guarded["stats"]
    assert s["epochs_run"] == [4, 1, 4], s
    assert guarded["adam_t"] == off["adam_t"] == 12 and one["adam_t"] == 3                 # Adam's step count stays the population's
    for name in ("flat", "adam_m", "adam_v"):
        assert torch.equal(_bits(guarded[name][1]), _bits(one[name][1])), name            # stopped after epoch 1: what one epoch leaves
        assert not torch.equal(_bits(guarded[name][1]), _bits(off[name][1])), name
        for m in (0, 2):                                                                   # the others: as without a target
            assert torch.equal(_bits(guarded[name][m]), _bits(off[name][m])), (name, m)
    assert guarded["live"][1, 0] == 0.0 and torch.equal(guarded["live"][1, 1:], guarded["hyper"][1, 1:])
    assert torch.equal(guarded["live"][0], guarded["hyper"][0]) and torch.equal(guarded["live"][2], guarded["hyper"][2])
    assert not (s["approx_kl"][1] <= 1.5 * TARGET) and s["approx_kl"][0] <= 1.5 * TARGET and s["approx_kl"][2] <= 1.5 * TARGET
    assert one["stats"]["epochs_run"] == [1, 1, 1]                                         # (epochs = 1: "never stopped" reads 1 too)


N_ENVS, HORIZON = 256, 8


def _ppo_run(seed=2, env_seed=42, iters=1, **kw):
    env = _env(N_ENVS, env_seed)
    agent = PPO(env, horizon=HORIZON, seed=seed, **kw)
    stats = [agent.iterate() for _ in range(iters)]
    torch.cuda.synchronize()
    out = {"flat": agent.flat.clone(), "adam_m": agent.adam_m.clone(), "adam_v": agent.adam_v.clone(), "adam_t": agent.adam_t,
           "stats": stats[-1]}
    env.close()
    return out


def _same(a, b, names=("flat", "adam_m", "adam_v")):
    return all(torch.equal(_bits(a[n]), _bits(b[n])) for n in names)


@pytest.mark.gpu
def test_ppo_with_a_target_nobody_reaches_is_ppo():
    plain = _ppo_run(iters=2)
    assert sorted(plain["stats"]) == ["clip_frac", "entropy", "mean_step_reward", "pg", "vf"]
    for kw in ({"diagnostics": True}, {"target_kl": 1e9}, {"target_kl": 1e9, "diag_rows": 2}):
        got = _ppo_run(iters=2, **kw)
        assert _same(got, plain) and got["adam_t"] == plain["adam_t"], kw
        assert sorted(set(got["stats"]) - set(plain["stats"])) == NEW_KEYS
        assert got["stats"]["epochs_run"] == 4 and got["stats"]["nonfinite"] == 0 and got["stats"]["approx_kl"] >= 0.0, got["stats"]
        assert all(got["stats"][k] == plain["stats"][k] for k in plain["stats"])


@pytest.mark.gpu
def test_ppo_with_a_tiny_target_stops_after_the_first_epoch():
    one, tiny, plain = _ppo_run(epochs=1), _ppo_run(target_kl=1e-12), _ppo_run()
    assert tiny["stats"]["epochs_run"] == 1 and tiny["stats"]["approx_kl"] > 1.5e-12
    assert _same(tiny, one) and not _same(tiny, plain)
    assert tiny["adam_t"] == plain["adam_t"] and one["adam_t"] * 4 == tiny["adam_t"]      # the step count goes on


@pytest.mark.gpu
def test_ppo_under_a_target_follows_attributes_changed_after_construction():
    """lr, clip and ent_coef are read at every update, as the unguarded step reads them: a schedule that sets agent.lr is obeyed, and
    lr = 0 is gradient-only without a step of Adam's count."""
    got = []
    for kw in ({}, {"target_kl": 1e9}):
        env = _env(N_ENVS, 45)
        agent = PPO(env, horizon=HORIZON, seed=6, **kw)
        agent.iterate()
        agent.lr, agent.clip, agent.ent_coef = 3e-4, 0.1, 0.02
        stats = agent.iterate()
        t_before, flat_before = agent.adam_t, agent.flat.clone()
        agent.lr = 0.0
        agent.iterate()
        torch.cuda.synchronize()
        assert agent.adam_t == t_before and torch.equal(_bits(agent.flat), _bits(flat_before)), kw
        got.append({"flat": agent.flat.clone(), "adam_m": agent.adam_m.clone(), "adam_v": agent.adam_v.clone(), "stats": stats})
        if kw:
            assert agent.hyper[0, :3].tolist() == torch.tensor([0.0, 0.1, 0.02]).tolist()
        env.close()
    assert _same(got[1], got[0])
    assert all(got[1]["stats"][k] == got[0]["stats"][k] for k in got[0]["stats"])


@pytest.mark.gpu
@pytest.mark.parametrize("option", ["normalize_obs", "policy_in_step"])
def test_the_other_options_run_with_the_guard(option):
    plain = _ppo_run(iters=2, **{option: True})
    got = _ppo_run(iters=2, target_kl=1e9, **{option: True})
    assert _same(got, plain)
    assert got["stats"]["epochs_run"] == 4 and np.isfinite(got["stats"]["approx_kl"]) and got["stats"]["explained_variance"] <= 1.0
    stopped = _ppo_run(iters=2, target_kl=1e-12, **{option: True})
    assert stopped["stats"]["epochs_run"] == 1 and not _same(stopped, plain)


def _resume(make, names=("flat", "adam_m", "adam_v", "obs")):
    env, a = make()
    for _ in range(2):
        a.iterate()
    sd = a.state_dict()
    want_stats = [a.iterate() for _ in range(2)]
    torch.cuda.synchronize()
    want, want_t = {n: getattr(a, n).clone() for n in names}, a.adam_t
    env.close()
    env2, b = make()
    b.iterate()                                                          # (another state: everything comes from the checkpoint)
    b.load_state_dict(sd)
    got_stats = [b.iterate() for _ in range(2)]
    torch.cuda.synchronize()
    for n in names:
        assert torch.equal(_bits(getattr(b, n)), _bits(want[n])), n
    assert b.adam_t == want_t
    assert repr(got_stats) == repr(want_stats)                           # (repr: a NaN equals itself)
    return env2, b, sd


@pytest.mark.gpu
def test_ppo_resume_is_bit_for_bit_and_other_options_are_refused():
    def make():
        env = _env(N_ENVS, 43)
        return env, PPO(env, horizon=HORIZON, seed=4, target_kl=0.01, diag_rows=4)

    env, agent, sd = _resume(make)
    assert (sd["diagnostics"], sd["target_kl"], sd["diag_row_step"]) == (True, 0.01, 2)
    env.close()
    env = _env(N_ENVS, 43)
    plain = PPO(env, horizon=HORIZON, seed=4)
    assert sorted(set(sd) - set(plain.state_dict())) == ["diag_row_step", "diagnostics", "target_kl"]   # nothing else is new
    with pytest.raises(ValueError, match="target_kl"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="target_kl"):
        agent.load_state_dict(plain.state_dict())
    env.close()
    env = _env(N_ENVS, 43)
    other = PPO(env, horizon=HORIZON, seed=4, target_kl=0.02, diag_rows=4)
    with pytest.raises(ValueError, match="target_kl"):
        other.load_state_dict(sd)
    env.close()


@pytest.mark.gpu
def test_population_resume_is_bit_for_bit():
    def make():
        env = _env(N_ENVS, 44)
        return env, PopulationPPO(env, 4, horizon=HORIZON, seeds=[5, 6, 7, 8], lr=[1e-3, 0.03, 1e-3, 3e-4], target_kl=0.02)

    env, pop, sd = _resume(make)
    env.close()
    env = _env(N_ENVS, 44)
    plain = PopulationPPO(env, 4, horizon=HORIZON)
    assert "diagnostics" not in plain.state_dict() and "target_kl" not in plain.state_dict()
    with pytest.raises(ValueError, match="target_kl"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="target_kl"):
        pop.load_state_dict(plain.state_dict())
    env.close()
