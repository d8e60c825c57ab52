"""The learner's kernels against float64 where an MLP kernel can go wrong numerically: saturated units, the workload's
observation range, tile and workgroup edges, the clip quadrants one by one, Adam step by step, GAE at the env's magnitudes.

pcc_policy_act, pcc_ppo_minibatch_step (ppo_grad_mfma_kernel, ppo_grad_tiled_kernel, ppo_adam_kernel), pcc_gae / pcc_gae_pop and
the tanh_fast / Gaussian head of csrc/pcc_policy_dev.h.  The reference is always torch in double on the CPU (MlpPolicy.double(),
ppo_loss, a plain GAE loop), never the code under test.  Every GPU test has a CPU twin (`..._cpu_twin`, unmarked): the same
inputs, the same conditions on them and the same bound, with torch's fp32 arithmetic on the CPU in the place of the kernel --
each bound is one a plain fp32 implementation meets, and each condition holds for the seeds used.  Two places where torch's own
autograd cannot stand in are stated at TorchFp32.grad (head="manual").

u = 2^-24 throughout.  PCC_NUMERICS_OUT=<file.json>: every test adds its maximum error next to its bound to that file
(the figures of profiles/r15_policy_numerics.json were collected that way: the GPU run's and the CPU twins' files, merged)."""
import copy
import ctypes
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch

from pcc_rl_amd.native import lib
from pcc_rl_amd.ppo import MlpPolicy, gae, ppo_loss

from test_ppo_shapes import _agent, _flat_grads, _p

U = 2.0 ** -24
GUARD = 64                                   # NaN floats on either side of every guarded output
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
_ids = lambda s: "%d-%d-%d" % s
F32 = lambda x: float(np.float32(x))         # what the C ABI receives for a float argument


def _record(check, shape, mode, impl, value, bound):
    key = "%s|%s|%s" % (check, _ids(shape) if isinstance(shape, tuple) else shape, mode)
    print("%-60s %-14s %.3e (bound %.3e)" % (key, impl, value, bound))
    path = os.environ.get("PCC_NUMERICS_OUT")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        row = data.setdefault(key, {})
        row["bound"] = bound
        row[impl] = max(value, row.get(impl, 0.0))
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------------------------------ inputs
_RANGES = {"typical": ((-0.5, 0.5), (1.0, 2.0), (0.0, 2.0)),
           "large": ((-1.0, 10.0), (1.0, 30.0), (0.0, 30.0)),
           "extreme": ((-1.0, 10.0), (1.0, 10000.0), (0.0, 1000.0))}   # pcc-rl_amd/metrics.py: the ratios' upper ends


def workload_obs(n, D, mode, generator):
    """[n, D] fp32: column k is metric k % 3 of (latency inflation, latency ratio, send ratio), uniform in the mode's range; in
    `extreme` a fifth of the entries sit at the range's maximum."""
    lo = torch.tensor([_RANGES[mode][k % 3][0] for k in range(D)])
    hi = torch.tensor([_RANGES[mode][k % 3][1] for k in range(D)])
    obs = lo + (hi - lo) * torch.rand(n, D, generator=generator)
    if mode == "extreme":
        obs = torch.where(torch.rand(n, D, generator=generator) < 0.2, hi.expand(n, D), obs)
    return obs.float().contiguous()


def deep_rows(pol64, n, D, generator):
    """4 n `extreme` rows, of which those are kept whose first-layer pre-activations of BOTH networks all have |s| >= 20 in
    float64: every first-layer unit is +-1 exactly in fp32.  Returns (rows, kept share): the caller asserts len(rows) >= n."""
    cand = workload_obs(4 * n, D, "extreme", generator)
    keep = torch.ones(4 * n, dtype=torch.bool)
    for net in (pol64.pi, pol64.vf):
        s = cand.double() @ net[0].weight.detach().T + net[0].bias.detach()
        keep &= (s.abs() >= 20.0).all(dim=1)
    return cand[keep].contiguous(), float(keep.double().mean())


def regime_obs(pol64, n, D, mode, generator):
    """`typical` / `large` rows, `deep` rows, or `mixed`: half `large`, half `deep`, shuffled.  Asserts deep_rows' condition."""
    if mode in ("typical", "large"):
        return workload_obs(n, D, mode, generator)
    n_deep = n if mode == "deep" else n - n // 2
    rows, share = deep_rows(pol64, n_deep, D, generator)
    assert len(rows) >= n_deep, "deep_rows kept %d of %d candidates (share %.2f), %d needed" % (len(rows), 4 * n_deep, share, n_deep)
    rows = rows[:n_deep]
    if mode == "mixed":
        rows = torch.cat([rows, workload_obs(n // 2, D, "large", generator)])
        rows = rows[torch.randperm(n, generator=generator)]
    return rows.contiguous()


def _policy(shape, seed=5, log_std=0.0):
    D, h1, h2 = shape
    torch.manual_seed(seed)
    pol = MlpPolicy(D, 1, (h1, h2))
    with torch.no_grad():
        pol.log_std.fill_(log_std)
    return pol


def _double(pol):
    D = pol.pi[0].in_features
    pol64 = MlpPolicy(D, 1, pol.hidden).double()
    pol64.load_state_dict({k: v.double() for k, v in pol.state_dict().items()})
    return pol64


def _logp64(pol64, obs, act):
    with torch.no_grad():
        return pol64.dist(obs.double()).log_prob(act.double().reshape(-1, 1)).sum(-1)


def _n_net(D, h1, h2):
    return h1 * D + h1 + h2 * h1 + h2 + h2 + 1


# ---------------------------------------------------------------------------------------------------------------- backends
def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _guarded(rows, n, dev):
    """`rows` output rows of n floats each with GUARD NaN floats on either side: (buffer, the views the kernel writes)."""
    buf = torch.full((rows, n + 2 * GUARD), float("nan"), device=dev)
    return buf, [buf[k, GUARD:GUARD + n] for k in range(rows)]


def _guards_untouched(buf, n):
    b = buf.cpu()
    return bool(torch.isnan(b[:, :GUARD]).all() and torch.isnan(b[:, GUARD + n:]).all())


class Kernel(object):
    """The HIP library through its C ABI; everything comes back as CPU tensors."""
    name = "gpu"

    def __init__(self):
        self.dev = torch.device("cuda:0")

    def act(self, pol, obs, noise):
        """(mean, act, logp, value) of pcc_policy_act, each output row between NaN guards that must stay NaN."""
        D, (h1, h2), n = obs.shape[1], pol.hidden, obs.shape[0]
        o, par = obs.to(self.dev).contiguous(), pol.flat_params().to(self.dev)
        nz = None if noise is None else noise.to(self.dev).contiguous()
        buf, outs = _guarded(4, n, self.dev)
        rc = lib().pcc_policy_act(_p(o), n, D, _p(par), h1, h2, _p(nz), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _stream(self.dev))
        torch.cuda.synchronize()
        assert rc == 0
        assert _guards_untouched(buf, n), "pcc_policy_act wrote outside its %d output rows" % n
        return [x.cpu().clone() for x in outs]

    def grad(self, pol, obs, act, logp_old, adv, ret, perm, start, count, clip=0.2, ent_coef=0.01, head=None):
        """pcc_ppo_minibatch_step with lr = 0: (gradient, stats)."""
        D, (h1, h2), n = obs.shape[1], pol.hidden, obs.shape[0]
        assert 0 <= start and start + count <= (n if perm is None else perm.numel()) and (perm is None or int(perm.max()) < n)
        dev = self.dev
        t = [x.to(dev).contiguous() for x in (obs, act.reshape(n), logp_old, adv, ret)]
        pm = None if perm is None else perm.to(dev).contiguous()
        par = pol.flat_params().to(dev)
        g, stats = torch.full((par.numel(),), float("nan"), device=dev), torch.full((4,), float("nan"), device=dev)
        scratch = torch.empty(lib().pcc_ppo_scratch_floats(D, h1, h2), device=dev)
        rc = lib().pcc_ppo_minibatch_step(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), _p(t[4]), _p(pm), start, count, D, h1, h2, _p(par),
                                          None, None, 1, 0.0, 0.9, 0.999, 1e-5, clip, ent_coef, _p(scratch), _p(g), _p(stats), _stream(dev))
        torch.cuda.synchronize()
        assert rc == 0
        return g.cpu(), stats.cpu().tolist()

    def adam_trace(self, shape, data, windows, t0=0, seed=7):
        """len(windows) consecutive optimiser steps of a fresh agent (adam_t starting at t0): per call the step number, grad_out, and
        the moments and parameters before and after."""
        dev = self.dev
        agent = _agent(shape, dev, seed=seed)
        agent.adam_t = t0
        obs, act, logp, adv, ret = [x.to(dev).contiguous() for x in data]
        g = torch.zeros_like(agent.flat)
        out = []
        for start, count in windows:
            before = [x.detach().cpu().clone() for x in (agent.adam_m, agent.adam_v, agent.flat)]
            agent.minibatch_step_fused(obs, act.reshape(-1), logp, adv, ret, None, start, count, grad_out=g)
            torch.cuda.synchronize()
            after = [x.detach().cpu().clone() for x in (agent.adam_m, agent.adam_v, agent.flat)]
            out.append((agent.adam_t, g.cpu().clone(), before, after))
        return out

    def gae(self, rew, val, done, last, gamma, lam):
        dev = self.dev
        T, N = rew.shape
        r, v, d, lv = rew.to(dev).contiguous(), val.to(dev).contiguous(), done.to(dev).to(torch.uint8).contiguous(), last.to(dev).contiguous()
        buf, (adv, ret) = _guarded(2, T * N, dev)
        rc = lib().pcc_gae(_p(r), _p(v), _p(d), _p(lv), T, N, gamma, lam, _p(adv), _p(ret), _stream(dev))
        torch.cuda.synchronize()
        assert rc == 0 and _guards_untouched(buf, T * N)
        return adv.cpu().reshape(T, N).clone(), ret.cpu().reshape(T, N).clone()

    def gae_pop(self, rew, val, done, last, hyper):
        dev = self.dev
        T, N = rew.shape
        r, v, d, lv = rew.to(dev).contiguous(), val.to(dev).contiguous(), done.to(dev).to(torch.uint8).contiguous(), last.to(dev).contiguous()
        hy = hyper.to(dev).contiguous()
        buf, (adv, ret) = _guarded(2, T * N, dev)
        rc = lib().pcc_gae_pop(_p(r), _p(v), _p(d), _p(lv), T, N, hy.shape[0], _p(hy), _p(adv), _p(ret), _stream(dev))
        torch.cuda.synchronize()
        assert rc == 0
        assert _guards_untouched(buf, T * N), "pcc_gae_pop wrote outside adv_out / ret_out"
        return adv.cpu().reshape(T, N).clone(), ret.cpu().reshape(T, N).clone()


def _manual_head(p, o, a, old, A, R, count, clip, ent_coef):
    """The objective's derivative with respect to log-probability and value written out (as the kernels have it), the networks by
    torch's fp32 autograd; the entropy term subtracted from the log_std entry once."""
    mu, v, ls = p.pi(o).squeeze(-1), p.value(o), p.log_std
    z = (a - mu) / ls.exp()
    logp = -0.5 * z * z - ls - HALF_LOG_2PI
    with torch.no_grad():
        ratio = (logp - old).exp()
        s1, s2 = ratio * A, ratio.clamp(1 - clip, 1 + clip) * A
        dlp = torch.where(s1 <= s2, -A * ratio / count, torch.zeros_like(A))
        dv = (v - R) / count
        stats = [float(torch.min(s1, s2).mean()), float((v - R).pow(2).mean()),
                 float(((ratio < 1 - clip) | (ratio > 1 + clip)).float().mean()), 0.0]
    torch.autograd.backward([logp, v], [dlp, dv])
    with torch.no_grad():
        p.log_std.grad -= ent_coef
    return stats


class TorchFp32(object):
    """torch's fp32 arithmetic on the CPU in the place of each kernel."""
    name = "torch_fp32_cpu"

    def act(self, pol, obs, noise):
        with torch.no_grad():
            d = pol.dist(obs)
            mean = d.mean.squeeze(-1)
            a = mean if noise is None else mean + pol.log_std.exp() * noise
            return [mean, a, d.log_prob(a.reshape(-1, 1)).sum(-1), pol.value(obs)]

    def grad(self, pol, obs, act, logp_old, adv, ret, perm, start, count, clip=0.2, ent_coef=0.01, head=None):
        """fp32 autograd of ppo_loss on the selected rows.  head="manual" (_manual_head) in the two cases where torch's autograd
        cannot stand in for a plain fp32 implementation: a ratio that overflows to inf in fp32 (exp's backward multiplies the
        incoming 0 by its inf output: NaN), and the statement that the log_std entry is exactly -ent_coef (autograd sums `count`
        roundings of -ent_coef / count)."""
        idx = torch.arange(start, start + count) if perm is None else perm[start:start + count]
        p = copy.deepcopy(pol)
        o, a, old, A, R = obs[idx], act.reshape(-1)[idx], logp_old[idx], adv[idx], ret[idx]
        if head == "manual":
            stats = _manual_head(p, o, a, old, A, R, count, clip, ent_coef)
        else:
            loss, pg, vf, _ = ppo_loss(p, o, a.reshape(-1, 1), old, A, R, clip, ent_coef)
            loss.backward()
            with torch.no_grad():
                ratio = (p.dist(o).log_prob(a.reshape(-1, 1)).sum(-1) - old).exp()
                frac = float(((ratio < 1 - clip) | (ratio > 1 + clip)).float().mean())
            stats = [-float(pg.detach()), 2.0 * float(vf.detach()), frac, 0.0]
        return _flat_grads(p).detach().clone(), stats

    def adam_trace(self, shape, data, windows, t0=0, seed=7):
        """ppo_adam_kernel's arithmetic in torch fp32 (scalars rounded to fp32, the bias corrections by float32 pow) on gradients
        from fp32 autograd."""
        pol = _policy(shape, seed)
        flat = pol.share_flat()
        m, v, t = torch.zeros_like(flat), torch.zeros_like(flat), t0
        f = np.float32
        b1, b2, eps, lr = F32(0.9), F32(0.999), F32(1e-5), F32(1e-3)
        out = []
        for start, count in windows:
            g, _ = self.grad(pol, *data, None, start, count, head="manual")
            t += 1
            before = [m.clone(), v.clone(), flat.detach().clone()]
            bias1 = float(f(1) - np.power(f(b1), f(t), dtype=f))
            bias2_sqrt = float(np.sqrt(f(1) - np.power(f(b2), f(t), dtype=f), dtype=f))
            with torch.no_grad():
                m = b1 * m + (1.0 - b1) * g
                v = b2 * v + (1.0 - b2) * g * g
                denom = v.sqrt() / bias2_sqrt + eps
                flat -= F32(f(lr) / f(bias1)) * (m / denom)
            out.append((t, g, before, [m.clone(), v.clone(), flat.detach().clone()]))
        return out

    def gae(self, rew, val, done, last, gamma, lam):
        return gae(rew, val, done, last, gamma, lam)

    def gae_pop(self, rew, val, done, last, hyper):
        T, N = rew.shape
        K = hyper.shape[0]
        n_m = N // K
        adv, ret = torch.empty_like(rew), torch.empty_like(rew)
        for k in range(K):
            sl = slice(k * n_m, (k + 1) * n_m)
            adv[:, sl], ret[:, sl] = gae(rew[:, sl], val[:, sl], done[:, sl], last[sl], float(hyper[k, 3]), float(hyper[k, 4]))
        return adv, ret


def both(fn):
    """The check `fn(impl, ...)` as a GPU test and as its CPU twin."""
    def gpu(*a, **k):
        fn(Kernel(), *a, **k)

    def twin(*a, **k):
        fn(TorchFp32(), *a, **k)
    gpu.__name__, twin.__name__ = "test_" + fn.__name__, "test_%s_cpu_twin" % fn.__name__
    gpu.__doc__ = twin.__doc__ = fn.__doc__
    sig = inspect.signature(fn)
    gpu.__signature__ = twin.__signature__ = sig.replace(parameters=list(sig.parameters.values())[1:])   # (pytest reads the parameters' names)
    marks = getattr(fn, "pytestmark", [])
    gpu.pytestmark, twin.pytestmark = marks + [pytest.mark.gpu.mark], list(marks)
    return gpu, twin


# ------------------------------------------------------------------------------------------ 1. tanh_fast over its whole range
TANH_BOUND = 2 * 2.0 ** -20   # two tanh_fast in a row, each <= 16 u = 2^-20 (DESIGN.md section 9 has the derivation)


def _tanh_points():
    special = [0.0, 1e-8, 1e-3, 44.3, 44.4, 88.7, 88.8, 1e4, 1e6]
    x = torch.cat([torch.linspace(-100.0, 100.0, 4096), torch.tensor(special), -torch.tensor(special)]).float()
    return x


def _tanh_policy(shape):
    """Every weight zero except W1[0][0] = W2[0][0] = W3[0] = 1 in both networks: mean = value = tanh(tanh(obs[0]))."""
    D, h1, h2 = shape
    pol = MlpPolicy(D, 1, (h1, h2))
    with torch.no_grad():
        for prm in pol.parameters():
            prm.zero_()
        for net in (pol.pi, pol.vf):
            net[0].weight[0, 0] = net[2].weight[0, 0] = net[4].weight[0, 0] = 1.0
    return pol


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 32, 16)], ids=_ids)   # the tiled forward; the fixed forward
def tanh_sweep(impl, shape):
    """tanh(tanh(x)) through pcc_policy_act over [-100, 100], across exp's overflow and underflow and far outside: finite, inside
    +-tanh(1), and within 2 x 2^-20 of float64."""
    pol = _tanh_policy(shape)
    x = _tanh_points()
    obs = torch.zeros(x.numel(), shape[0])
    obs[:, 0] = x
    mean, act, logp, value = impl.act(pol, obs, None)
    want = torch.tanh(torch.tanh(x.double()))
    worst = 0.0
    for name, out in (("mean", mean), ("value", value)):
        assert torch.isfinite(out).all(), name
        assert float(out.abs().max()) <= math.tanh(1.0) + TANH_BOUND, name
        err = (out.double() - want).abs()
        worst = max(worst, float(err.max()))
        assert float(err.max()) <= TANH_BOUND, (name, float(err.max()), float(x[err.argmax()]))
    assert torch.equal(act, mean) and torch.isfinite(logp).all()
    _record("tanh_fast_sweep", shape, "x in [-1e6, 1e6]", impl.name, worst, TANH_BOUND)


test_tanh_sweep, test_tanh_sweep_cpu_twin = both(tanh_sweep)

# ------------------------------------------------------------------------------------------------ 2. forward against float64
FWD_SHAPES = [(30, 32, 16), (30, 20, 10), (36, 64, 32), (120, 64, 64), (45, 48, 24)]   # fixed, generic (tanhf), tiled x 3
EDGE_ROWS = [31, 32, 33, 95, 96, 97, 127, 128, 129, 255, 256, 257]


def _big_rows(shape):
    """The counts from which a wavefront of policy_act_tiled_kernel walks a second tile: 128 workgroups x 3 (obs > 64 and h1 > 32)
    or 4 wavefronts x 32 rows, plus one row and plus a tile and a row."""
    full = 128 * (3 if shape[0] > 64 and shape[1] > 32 else 4) * 32
    return [full + 1, full + 33]


@pytest.mark.parametrize("mode", ["typical", "large", "deep"])
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=_ids)
def forward_matches_float64(impl, shape, mode):
    """pcc_policy_act on workload-range observations at every tile and workgroup edge and past the capped grid: mean and value
    within 1e-5 of float64, the log-probability within the bounds of tests/test_ppo_shapes.py (1e-4; 1e-5 where the draw is 0),
    the action within 4 u (|mean| + |sigma noise|) of mean + exp(log_std) noise, nothing written outside the output rows."""
    D = shape[0]
    pol = _policy(shape, seed=1)
    pol64 = _double(pol)
    g = torch.Generator().manual_seed(100 + D)
    rows_all = EDGE_ROWS + _big_rows(shape)
    obs = regime_obs(pol64, max(rows_all), D, mode, g)
    noise = torch.randn(max(rows_all), generator=g)
    noise[0], noise[1], noise[2] = 0.0, 6.0, -6.0
    with torch.no_grad():
        mean64, value64 = pol64.pi(obs.double()).squeeze(-1), pol64.value(obs.double())
    worst, worst_lp, worst_act = 0.0, 0.0, 0.0
    for rows in rows_all:
        for log_std in (-3.0, 0.0, 1.0):
            with torch.no_grad():
                pol.log_std.fill_(log_std)
            mean, act, logp, value = impl.act(pol, obs[:rows].contiguous(), noise[:rows])
            for out in (mean, act, logp, value):
                assert out.shape == (rows,) and torch.isfinite(out).all()
            e_mean, e_val = (mean.double() - mean64[:rows]).abs().max().item(), (value.double() - value64[:rows]).abs().max().item()
            worst = max(worst, e_mean, e_val)
            assert e_mean <= 1e-5 and e_val <= 1e-5, (rows, log_std, e_mean, e_val)
            nz = noise[:rows].double()
            e_lp = (logp.double() - (-0.5 * nz * nz - log_std - HALF_LOG_2PI)).abs()
            worst_lp = max(worst_lp, e_lp.max().item())
            assert e_lp.max().item() <= 1e-4 and e_lp[nz == 0].max().item() <= 1e-5, (rows, log_std, e_lp.max().item())
            sn = math.exp(log_std) * nz
            e_act = (act.double() - (mean.double() + sn)).abs() / (4 * U * (mean.double().abs() + sn.abs()))
            worst_act = max(worst_act, e_act.max().item())
            assert e_act.max().item() <= 1.0, (rows, log_std, e_act.max().item())
    _record("forward mean/value", shape, mode, impl.name, worst, 1e-5)
    _record("forward logp", shape, mode, impl.name, worst_lp, 1e-4)
    _record("forward act / (4u(|mean|+|sigma noise|))", shape, mode, impl.name, worst_act, 1.0)


test_forward_matches_float64, test_forward_matches_float64_cpu_twin = both(forward_matches_float64)

# ------------------------------------------------------------------------------------- 3. gradient against float64 autograd
GRAD_SHAPES = [(30, 32, 16), (12, 32, 16), (36, 64, 32), (120, 64, 64), (7, 20, 10), (45, 48, 24)]   # MFMA x 2, tiled x 4
CLIP, ENT = 0.2, 0.01


def _samples(pol64, obs, g, spread=0.15, zeros=True):
    """act / logp_old / adv / ret for the rows `obs` like tests/test_ppo_shapes.py's: log-probabilities near the policy's own
    (float64), so ratios around 1 with some clipped; every 97th advantage 0 unless zeros=False."""
    n = obs.shape[0]
    act = 0.5 * torch.randn(n, generator=g)
    adv = torch.randn(n, generator=g)
    adv[adv == 0] = 1.0
    if zeros:
        adv[::97] = 0.0
    ret = 2.0 * torch.randn(n, generator=g)
    logp = (_logp64(pol64, obs, act) + spread * torch.randn(n, generator=g).double()).float()
    return act, logp, adv, ret


def _reference(pol, obs, act, logp_old, adv, ret, idx, clip=CLIP, ent_coef=ENT):
    """float64 autograd of ppo_loss on rows idx of the fp32 inputs: (gradient, policy term, value term, clipped fraction)."""
    pol64 = _double(pol)
    o, a = obs[idx].double(), act.reshape(-1, 1)[idx].double()
    loss, pg, vf, _ = ppo_loss(pol64, o, a, logp_old[idx].double(), adv[idx].double(), ret[idx].double(), clip, ent_coef)
    loss.backward()
    with torch.no_grad():
        ratio = (pol64.dist(o).log_prob(a).sum(-1) - logp_old[idx].double()).exp()
    return _flat_grads(pol64).detach(), float(pg.detach()), float(vf.detach()), ratio


def _assert_grad(g, stats, want, pg, vf, what):
    """The bound of tests/test_ppo.py and tests/test_ppo_shapes.py, and their statistics bounds; returns err / max|want|."""
    assert torch.isfinite(g).all() and all(math.isfinite(s) for s in stats), what
    err, scale = (g.double() - want).abs().max().item(), want.abs().max().item()
    bound = 1e-5 * scale + 1e-7
    print("%s: err %.3e bound %.3e stats %s" % (what, err, bound, stats))
    assert err <= bound, (what, err, bound)
    assert abs(-stats[0] - pg) < 1e-4 * max(1.0, abs(pg)) and abs(0.5 * stats[1] - vf) < 1e-4 * max(1.0, vf), (what, stats, pg, vf)
    assert stats[3] == 0.0
    return err / bound


def _first_layer(shape):
    """Indices of W1 and b1 of both networks in the flat gradient."""
    D, h1, h2 = shape
    one = torch.arange(h1 * D + h1)
    return torch.cat([one, one + _n_net(D, h1, h2) + 1])


@pytest.mark.parametrize("count", [64, 3333])
@pytest.mark.parametrize("mode", ["large", "deep", "mixed"])
@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=_ids)
def gradient_in_the_saturated_regime(impl, shape, mode, count):
    """(a) observations of the workload's range -- units in the transition, units saturated to +-1, the two mixed: the existing
    bound.  In `deep` every first-layer unit is +-1 exactly, so W1's and b1's gradients are below 1e-7 (float64: < 1e-12)."""
    D = shape[0]
    pol = _policy(shape, log_std=-0.4)
    pol64 = _double(pol)
    g = torch.Generator().manual_seed(7 * D + count)
    n, start = count + 10, 5
    obs = regime_obs(pol64, n, D, mode, g)
    act, logp, adv, ret = _samples(pol64, obs, g)
    perm = torch.randperm(n, generator=g)
    grad, stats = impl.grad(pol, obs, act, logp, adv, ret, perm, start, count, CLIP, ENT)
    want, pg, vf, ratio = _reference(pol, obs, act, logp, adv, ret, perm[start:start + count])
    frac = ((ratio < 1 - CLIP) | (ratio > 1 + CLIP)).double().mean().item()
    assert 0.0 < frac < 1.0 and 0.0 < stats[2] < 1.0          # some ratios clipped, not all
    rel = _assert_grad(grad, stats, want, pg, vf, "%s %s %d" % (shape, mode, count))
    if mode == "deep":
        fl = _first_layer(shape)
        assert want[fl].abs().max().item() < 1e-12
        assert grad[fl].abs().max().item() <= 1e-7, grad[fl].abs().max().item()
    _record("gradient err / bound", shape, "%s count %d" % (mode, count), impl.name, rel, 1.0)


test_gradient_in_the_saturated_regime, test_gradient_in_the_saturated_regime_cpu_twin = both(gradient_in_the_saturated_regime)

EDGE_COUNTS = [31, 32, 33, 63, 65, 95, 96, 97, 127, 128, 129]   # tiles of 32 / 64 samples, workgroups of 96 / 128


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=_ids)
def gradient_at_tile_and_workgroup_edges(impl, shape):
    """(b) minibatch counts one either side of every tile and workgroup size, inside the rollout (start = 3, n = count + 7) and
    ending exactly at its end, with and without perm: the existing bound."""
    D = shape[0]
    pol = _policy(shape, log_std=-0.4)
    pol64 = _double(pol)
    g = torch.Generator().manual_seed(11 * D)
    worst = 0.0
    for count in EDGE_COUNTS:
        n = count + 7
        obs = workload_obs(n, D, "typical", g)
        act, logp, adv, ret = _samples(pol64, obs, g)
        for start in (3, n - count):
            for with_perm in (True, False):
                perm = torch.randperm(n, generator=g) if with_perm else None
                idx = perm[start:start + count] if with_perm else torch.arange(start, start + count)
                grad, stats = impl.grad(pol, obs, act, logp, adv, ret, perm, start, count, CLIP, ENT)
                want, pg, vf, _ = _reference(pol, obs, act, logp, adv, ret, idx)
                worst = max(worst, _assert_grad(grad, stats, want, pg, vf, "%s count %d start %d perm %s" % (shape, count, start, with_perm)))
    _record("gradient err / bound", shape, "typical, edge counts", impl.name, worst, 1.0)


test_gradient_at_tile_and_workgroup_edges, test_gradient_at_tile_and_workgroup_edges_cpu_twin = both(gradient_at_tile_and_workgroup_edges)


@pytest.mark.parametrize("shape", [(30, 32, 16), (36, 64, 32), (7, 20, 10)], ids=_ids)
def nothing_outside_the_minibatch_is_used(impl, shape):
    """(c) the same call again with every row that is not one of the `count` selected samples overwritten with NaN: the same
    bits, all finite."""
    D = shape[0]
    pol = _policy(shape, log_std=-0.4)
    g = torch.Generator().manual_seed(13 * D)
    n, start, count = 150, 3, 97
    obs = workload_obs(n, D, "typical", g)
    act, logp, adv, ret = _samples(_double(pol), obs, g)
    perm = torch.randperm(n, generator=g)
    g1, s1 = impl.grad(pol, obs, act, logp, adv, ret, perm, start, count)
    out = torch.ones(n, dtype=torch.bool)
    out[perm[start:start + count]] = False
    assert int(out.sum()) == n - count
    obs, act, logp, adv, ret = [x.clone() for x in (obs, act, logp, adv, ret)]
    for x in (obs, act, logp, adv, ret):
        x[out] = float("nan")
    g2, s2 = impl.grad(pol, obs, act, logp, adv, ret, perm, start, count)
    assert torch.isfinite(g1).all() and all(math.isfinite(s) for s in s1) and g1.abs().max() > 0
    assert torch.equal(g1, g2) and s1 == s2


test_nothing_outside_the_minibatch_is_used, test_nothing_outside_the_minibatch_is_used_cpu_twin = both(nothing_outside_the_minibatch_is_used)

EXACT_COUNT = 300   # (no multiple of a tile; see the condition on it in exact_statements)


@pytest.mark.parametrize("shape", [(30, 32, 16), (36, 64, 32), (7, 20, 10)], ids=_ids)
def exact_statements(impl, shape):
    """(d) the clip quadrants one by one, and what the objective makes exactly zero."""
    D, h1, h2 = shape
    N = _n_net(D, h1, h2)
    pol = _policy(shape, log_std=-0.4)
    pol64 = _double(pol)
    g = torch.Generator().manual_seed(17 * D)
    n, start, count = EXACT_COUNT + 10, 4, EXACT_COUNT
    # the clipped fraction is sum x fl(1 / count) in fp32: `== 1.0` asks of `count` that this product is exact
    assert np.float32(count) * (np.float32(1) / np.float32(count)) == np.float32(1)
    obs = workload_obs(n, D, "typical", g)
    act, logp, adv, ret = _samples(pol64, obs, g, zeros=False)
    perm = torch.randperm(n, generator=g)
    idx = perm[start:start + count]
    own = _logp64(pol64, obs, act)                             # the policy's own log-probabilities: ratio 1
    up, down = adv > 0, adv < 0
    assert bool((up | down).all())
    ent32 = torch.tensor(ENT, dtype=torch.float32)

    def run(logp_old, adv_, clip=CLIP, head=None, ret_=ret):
        grad, stats = impl.grad(pol, obs, act, logp_old, adv_, ret_, perm, start, count, clip, ENT, head=head)
        return grad, stats, _reference(pol, obs, act, logp_old, adv_, ret_, idx, clip)

    def pi_is_exactly_zero(grad, what):
        assert not grad[:N].any(), what                        # every pi-network entry is 0.0
        assert grad[N] == -ent32, (what, float(grad[N]))       # log_std: the entropy term alone
        assert grad[N + 1:].abs().max() > 0

    # zero advantages
    grad, stats, (want, pg, vf, _) = run(logp, torch.zeros(n), head="manual")
    pi_is_exactly_zero(grad, "adv = 0")
    assert stats[0] == 0.0
    _assert_grad(grad, stats, want, pg, vf, "%s adv = 0" % (shape,))
    # every ratio clipped against its advantage: ratio ~ e for A > 0, ~ 1 / e for A < 0
    clipped = (own - torch.where(up, 1.0, -1.0)).float()
    grad, stats, (want, pg, vf, ratio) = run(clipped, adv, head="manual")
    assert bool(((ratio[adv[idx] > 0] > 1 + CLIP).all()) and (ratio[adv[idx] < 0] < 1 - CLIP).all())
    pi_is_exactly_zero(grad, "all clipped")
    assert stats[2] == 1.0
    _assert_grad(grad, stats, want, pg, vf, "%s all clipped" % (shape,))
    # the mirrored signs: outside the clip range, but the min takes the unclipped term
    mirrored = (own + torch.where(up, 1.0, -1.0)).float()
    grad, stats, (want, pg, vf, ratio) = run(mirrored, adv)
    assert bool(((ratio[adv[idx] > 0] < 1 - CLIP).all()) and (ratio[adv[idx] < 0] > 1 + CLIP).all())
    assert stats[2] == 1.0 and want[:N].abs().max() > 0
    r1 = _assert_grad(grad, stats, want, pg, vf, "%s mirrored" % (shape,))
    # a clip range nothing reaches
    grad, stats, (want, pg, vf, _) = run(logp, adv, clip=1e9)
    assert stats[2] == 0.0
    r2 = _assert_grad(grad, stats, want, pg, vf, "%s clip 1e9" % (shape,))
    # a tenth of the samples with a ratio that overflows to inf / underflows (e^-100: below the smallest normal) in fp32, on the clipped side
    far = logp.clone()
    tenth = torch.zeros(n, dtype=torch.bool)
    tenth[perm[start:start + count:10]] = True
    far[tenth] = (own - torch.where(up, 100.0, -100.0)).float()[tenth]
    assert bool(torch.isinf((own.float() - far)[tenth & up].exp()).all()) and bool(((own.float() - far)[tenth & down].exp() < 2.0 ** -126).all())
    assert int((tenth & up).sum()) > 0 and int((tenth & down).sum()) > 0
    grad, stats, (want, pg, vf, ratio) = run(far, adv, head="manual")
    assert bool(torch.isfinite(ratio).all())
    r3 = _assert_grad(grad, stats, want, pg, vf, "%s ratio inf / 0" % (shape,))
    # the value network on its own forward's output: no value error
    value_out = impl.act(pol, obs, None)[3]
    grad, stats, _ = run(logp, adv, ret_=value_out)
    vf_abs = grad[N + 1:].abs().max().item()
    print("%s ret = value_out: max |vf gradient| %.3e, stats[1] %.3e" % (shape, vf_abs, stats[1]))
    assert vf_abs <= 1e-7 and 0.0 <= stats[1] <= 1e-10, (vf_abs, stats[1])
    _record("gradient err / bound", shape, "mirrored | clip 1e9 | ratio inf / 0", impl.name, max(r1, r2, r3), 1.0)
    _record("vf gradient at ret = value_out", shape, "typical", impl.name, vf_abs, 1e-7)


test_exact_statements, test_exact_statements_cpu_twin = both(exact_statements)


@pytest.mark.parametrize("shape", [(30, 32, 16), (30, 20, 10), (45, 48, 24)], ids=_ids)   # (30; 20, 10): forward tanhf, gradient tanh_fast
def rollout_to_update_hand_off(impl, shape):
    """(e) act_out and logp_out of pcc_policy_act fed straight into pcc_ppo_minibatch_step with the same parameters: no ratio is
    clipped, and the gradient is float64 autograd's at logp_old = the float64 log-probability of those actions (ratio exactly 1)."""
    D = shape[0]
    pol = _policy(shape, log_std=-1.0)
    pol64 = _double(pol)
    g = torch.Generator().manual_seed(19 * D)
    n, start, count = 264, 3, 257
    obs = workload_obs(n, D, "typical", g)
    noise = torch.randn(n, generator=g).clamp(-4.0, 4.0)
    noise[0], noise[1], noise[2] = 4.0, -4.0, 0.0
    _, act, logp, _ = impl.act(pol, obs, noise)
    _, _, adv, ret = _samples(pol64, obs, g, zeros=False)
    perm = torch.randperm(n, generator=g)
    grad, stats = impl.grad(pol, obs, act, logp, adv, ret, perm, start, count, CLIP, ENT)
    assert stats[2] == 0.0
    own = _logp64(pol64, obs, act)
    idx = perm[start:start + count]
    pol_ref = _double(pol)
    loss, pg, vf, _ = ppo_loss(pol_ref, obs[idx].double(), act.reshape(-1, 1)[idx].double(), own[idx], adv[idx].double(), ret[idx].double(), CLIP, ENT)
    loss.backward()
    rel = _assert_grad(grad, stats, _flat_grads(pol_ref).detach(), float(pg.detach()), float(vf.detach()), "%s hand-off" % (shape,))
    _record("gradient err / bound", shape, "rollout to update hand-off", impl.name, rel, 1.0)


test_rollout_to_update_hand_off, test_rollout_to_update_hand_off_cpu_twin = both(rollout_to_update_hand_off)

# ------------------------------------------------------------------------------------------------------ 4. Adam in isolation
B1, B2, EPS, LR = F32(0.9), F32(0.999), F32(1e-5), F32(1e-3)


def adam_step64(t, g, m0, v0):
    """torch.optim.Adam's step in float64 from fp32 inputs and fp32-rounded constants: (m, v, step(m, v))."""
    m = B1 * m0.double() + (1.0 - B1) * g.double()
    v = B2 * v0.double() + (1.0 - B2) * g.double() * g.double()
    return m, v, lambda m_, v_: LR / (1.0 - B1 ** t) * m_.double() / (v_.double().sqrt() / math.sqrt(1.0 - B2 ** t) + EPS)


def _assert_adam(t, g, before, after, what):
    """One call: the moments from grad_out and the moments before, the parameter step from the fp32 moments after.  Returns the
    largest step error as a fraction of its bound."""
    (m0, v0, p0), (m1, v1, p1) = before, after
    m64, v64, step = adam_step64(t, g, m0, v0)
    e_m = (m1.double() - m64).abs() - 4 * U * ((B1 * m0.double()).abs() + ((1.0 - B1) * g.double()).abs())
    assert e_m.max().item() <= 0.0, (what, "m", e_m.max().item())
    e_v = (v1.double() - v64).abs() - 6 * U * v64
    assert e_v.max().item() <= 0.0, (what, "v", e_v.max().item())
    want = step(m1, v1)
    rel = 8 * U + 2 * U * B1 ** t / (1.0 - B1 ** t) + U * B2 ** t / (1.0 - B2 ** t)
    bound = rel * want.abs() + U * torch.maximum(p0.abs(), p1.abs()).double()
    frac = ((p0.double() - p1.double() - want).abs() / bound).max().item()
    assert frac <= 1.0, (what, "step", frac)
    return frac


def _adam_data(shape, n=4096):
    D = shape[0]
    g = torch.Generator().manual_seed(3)
    obs = workload_obs(n, D, "typical", g)
    act, logp, adv, ret = _samples(_double(_policy(shape, seed=7)), obs, g, spread=0.1)
    return obs, act, logp, adv, ret


@pytest.mark.parametrize("shape", [(30, 32, 16), (36, 64, 32)], ids=_ids)
def adam_steps_match_their_float64_restatement(impl, shape):
    """200 consecutive optimiser steps on a rotating window of one rollout, each held against the float64 restatement from the
    call's own fp32 inputs; then one call at adam_step = 1 000 000."""
    data = _adam_data(shape)
    count = 1024
    windows = [((193 * k) % (4096 - count + 1), count) for k in range(200)]
    trace = impl.adam_trace(shape, data, windows)
    assert [r[0] for r in trace] == list(range(1, 201))
    fracs = {}
    for t, g, before, after in trace:
        assert g.abs().max() > 0 and not torch.equal(before[2], after[2])
        fracs[t] = _assert_adam(t, g, before, after, "%s t %d" % (shape, t))
    for t in (1, 2, 200):
        _record("adam step err / bound", shape, "t = %d" % t, impl.name, fracs[t], 1.0)
    _record("adam step err / bound", shape, "t = 1 .. 200", impl.name, max(fracs.values()), 1.0)
    (t, g, before, after), = impl.adam_trace(shape, data, [(5, count)], t0=999999)
    assert t == 1000000
    _record("adam step err / bound", shape, "t = 1000000", impl.name, _assert_adam(t, g, before, after, "%s t 1e6" % (shape,)), 1.0)


test_adam_steps_match_their_float64_restatement, test_adam_steps_match_their_float64_restatement_cpu_twin = \
    both(adam_steps_match_their_float64_restatement)


@pytest.mark.parametrize("shape", [(30, 32, 16), (36, 64, 32)], ids=_ids)
def adam_leaves_zero_gradient_rows_alone(impl, shape):
    """Zero advantages make every pi-network gradient exactly 0: with zero moments, m, v and the parameter keep their bits."""
    D, h1, h2 = shape
    N = _n_net(D, h1, h2)
    obs, act, logp, adv, ret = _adam_data(shape, 512)
    (t, g, before, after), = impl.adam_trace(shape, (obs, act, logp, torch.zeros_like(adv), ret), [(7, 300)])
    zero = g == 0
    assert bool(zero[:N].all()) and not bool(zero[N]) and not bool(zero[N + 1:].all())
    bits = lambda x: x.view(torch.int32)
    for b, a in zip(before, after):
        assert torch.equal(bits(a)[zero], bits(b)[zero])
    assert not torch.equal(after[2][~zero], before[2][~zero])
    _assert_adam(t, g, before, after, "%s adv = 0" % (shape,))


test_adam_leaves_zero_gradient_rows_alone, test_adam_leaves_zero_gradient_rows_alone_cpu_twin = both(adam_leaves_zero_gradient_rows_alone)


def test_adam_restatement_is_torch_adam_in_double():
    """The float64 restatement the Adam tests hold the kernel to is torch.optim.Adam's arithmetic: five steps in double."""
    g = torch.Generator().manual_seed(1)
    p = torch.nn.Parameter(torch.randn(257, generator=g, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=LR, betas=(B1, B2), eps=EPS)
    q, m, v = p.detach().clone(), torch.zeros(257, dtype=torch.float64), torch.zeros(257, dtype=torch.float64)
    for t in range(1, 6):
        grad = torch.randn(257, generator=g, dtype=torch.float64) * 10.0 ** float(t - 3)
        p.grad = grad.clone()
        opt.step()
        m, v, step = adam_step64(t, grad, m, v)
        q = q - step(m, v)
        st = opt.state[p]
        assert torch.allclose(st["exp_avg"], m, rtol=1e-13, atol=0) and torch.allclose(st["exp_avg_sq"], v, rtol=1e-13, atol=0)
        assert torch.allclose(p.detach(), q, rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------------------------------- 5. GAE against a float64 loop
def gae64(rew, val, done, last, gamma, lam):
    """The float64 recursion from fp32 inputs (gamma, lam as the ABI receives them), and next to it the running error bound
    E_t = gamma lam alive E_{t+1} + 4 u (|r_t| + gamma alive |v_{t+1}| + |v_t| + gamma lam alive |run_{t+1}|)."""
    gamma, lam = F32(gamma), F32(lam)
    T = rew.shape[0]
    r, v, lv = rew.double(), val.double(), last.double()
    adv, E = torch.zeros_like(r), torch.zeros_like(r)
    run, e, nxt = torch.zeros_like(lv), torch.zeros_like(lv), lv
    for t in range(T - 1, -1, -1):
        alive = 1.0 - done[t].double()
        e = gamma * lam * alive * e + 4 * U * (r[t].abs() + gamma * alive * nxt.abs() + v[t].abs() + gamma * lam * alive * run.abs())
        run = r[t] + gamma * nxt * alive - v[t] + gamma * lam * alive * run
        adv[t], E[t], nxt = run, e, v[t]
    return adv, adv + v, E


def _gae_inputs(T, N, pattern, seed):
    g = torch.Generator().manual_seed(seed)
    rew, val, last = 3.0 * torch.randn(T, N, generator=g), 20.0 * torch.randn(T, N, generator=g), 20.0 * torch.randn(N, generator=g)
    done = torch.zeros(T, N, dtype=torch.bool)
    if pattern == "every":
        done[:] = True
    elif pattern == "last":
        done[T - 1] = True
    elif pattern == "first":
        done[0] = True
    elif pattern == "bernoulli":
        done = torch.rand(T, N, generator=g) < 0.01
        assert bool(done.any()) and not bool(done.all())
    else:
        assert pattern == "none"
    return rew, val, done, last


def _assert_gae(adv, ret, rew, val, done, want_adv, want_ret, E, what):
    assert torch.isfinite(adv).all() and torch.isfinite(ret).all(), what
    f_adv = ((adv.double() - want_adv).abs() / (2 * E)).max().item()
    f_ret = ((ret.double() - want_ret).abs() / (2 * E + U * want_ret.abs())).max().item()
    assert f_adv <= 1.0 and f_ret <= 1.0, (what, f_adv, f_ret)
    assert torch.equal(ret, adv + val), what                   # bitwise: one fp32 addition
    every = done.all(dim=0)
    if bool(every.any()):
        assert torch.equal(adv[:, every], (rew - val)[:, every]), what
    return 2 * f_adv                                           # err / E_t


GAE_CASES = [(1, 1, (0.99, 0.95), "none"), (2, 255, (0.0, 0.95), "every"), (37, 256, (0.999, 0.0), "last"),
             (37, 257, (0.99, 0.95), "first"), (400, 1000, (1.0, 1.0), "bernoulli"), (400, 257, (0.99, 0.95), "none"),
             (37, 1000, (1.0, 1.0), "every")]


@pytest.mark.parametrize("T,N,gl,pattern", GAE_CASES, ids=lambda x: str(x).replace(" ", ""))
def gae_matches_the_float64_loop(impl, T, N, gl, pattern):
    """pcc_gae at the env's magnitudes (rewards ~ 3 N(0, 1), values ~ 20 N(0, 1)), at T = 1 and the episode length, N across the
    256-thread workgroup, the corner (gamma, lam) and done patterns: within twice the running bound; ret = adv + values and, with
    done on every step, adv = rewards - values bit for bit."""
    rew, val, done, last = _gae_inputs(T, N, pattern, 1000 * T + N)
    adv, ret = impl.gae(rew, val, done, last, gl[0], gl[1])
    want_adv, want_ret, E = gae64(rew, val, done, last, gl[0], gl[1])
    if pattern == "every":
        assert bool(done.all())
    f = _assert_gae(adv, ret, rew, val, done, want_adv, want_ret, E, (T, N, gl, pattern))
    _record("gae err / E_t", "T %d N %d" % (T, N), "gamma %g lam %g done %s" % (gl[0], gl[1], pattern), impl.name, f, 2.0)


test_gae_matches_the_float64_loop, test_gae_matches_the_float64_loop_cpu_twin = both(gae_matches_the_float64_loop)

_GL = [(0.99, 0.95), (1.0, 1.0), (0.0, 0.95), (0.999, 0.0)]


@pytest.mark.parametrize("members,N", [(4, 1028), (257, 257)], ids=["4x257", "257x1"])
def gae_pop_matches_the_float64_loop(impl, members, N):
    """pcc_gae_pop: every member's columns with its own (gamma, lam) row against the float64 loop, nothing written outside
    adv_out / ret_out: four members of 257 envs, and one env per member."""
    T = 37
    rew, val, done, last = _gae_inputs(T, N, "bernoulli", 77 + members)
    hyper = torch.zeros(members, 8)
    for k in range(members):
        hyper[k, 0], hyper[k, 1], hyper[k, 2] = 1e-3, 0.2, 0.01
        hyper[k, 3], hyper[k, 4] = _GL[k % 4]
    adv, ret = impl.gae_pop(rew, val, done, last, hyper)
    n_m = N // members
    worst = 0.0
    for k in range(members):
        sl = slice(k * n_m, (k + 1) * n_m)
        gamma, lam = _GL[k % 4]
        want_adv, want_ret, E = gae64(rew[:, sl], val[:, sl], done[:, sl], last[sl], gamma, lam)
        worst = max(worst, _assert_gae(adv[:, sl], ret[:, sl], rew[:, sl], val[:, sl], done[:, sl], want_adv, want_ret, E, (members, k)))
    _record("gae_pop err / E_t", "T %d N %d" % (T, N), "%d members" % members, impl.name, worst, 2.0)


test_gae_pop_matches_the_float64_loop, test_gae_pop_matches_the_float64_loop_cpu_twin = both(gae_pop_matches_the_float64_loop)
