#!/usr/bin/env python3
"""The PPO kernels' outputs on seeded inputs, one shape per kernel family, straight through the C ABI of ONE build of the
library, into a .pt file -- to compare two builds (GPU box):
   python tools/dump_ppo_outputs.py path/libpcc_sim.so out.pt          for each build, then
   python tools/dump_ppo_outputs.py --compare a.pt b.pt                torch.equal on every tensor
For every shape of SHAPES, on a seeded batch of 5 000 samples with a window of 4 097 from row 7 on (ragged last tiles of both 32
and 64 samples, more tiles than one workgroup walks; the first shape at 70 000 / 66 000, beyond the 512-block cap of the grid):
  - pcc_ppo_minibatch_step with lr = 0 and a permutation: gradient and statistics; the same with perm = NULL;
  - three consecutive pcc_ppo_minibatch_step calls with lr = 1e-3: params, adam_m, adam_v after them;
  - pcc_policy_act's four outputs;
  - pcc_gae at T = 5 over 1 000 envs, some dones set;
  - the three _pop entry points at 3 members x 257 rows (member boundaries inside a workgroup, a wavefront and a 32-sample tile),
    another row of hyper-parameters per member, one member with lr = 0: two optimiser steps.
Uses only symbols every build since the population entry points has."""
import ctypes, sys
import torch

SHAPES = [(30, 32, 16), (12, 32, 16),   # ppo_grad_mfma_kernel + policy_act_fixed_kernel
          (36, 32, 16),                 # policy_act_fixed_kernel + the tiled gradient, DP 64
          (30, 16, 8),                  # the generic policy_act_kernel + tiled DP 32
          (45, 48, 24),                 # tiled 64 / (64, 32)
          (120, 64, 64),                # tiled 128 / (64, 64)
          (1, 1, 1)]                    # all padding
K, ROWS, T = 3, 257, 5                  # the population: members, rows per member; the GAE's steps
HYPER = [[1e-3, 0.2, 0.01, 0.99, 0.95, 0, 0, 0], [0.0, 0.1, 0.0, 0.9, 0.8, 0, 0, 0], [3e-4, 0.3, 0.02, 0.999, 1.0, 0, 0, 0]]


def dump(path, out):
    L = ctypes.CDLL(path)
    L.pcc_ppo_scratch_floats.restype = ctypes.c_int
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    L.pcc_policy_act.argtypes = [vp, i64, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.pcc_ppo_minibatch_step.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, vp, vp, vp, i32, f32, f32, f32, f32,
                                         f32, f32, vp, vp, vp, vp]
    L.pcc_gae.argtypes = [vp, vp, vp, vp, i32, i64, f32, f32, vp, vp, vp]
    L.pcc_policy_act_pop.argtypes = [vp, i64, i32, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.pcc_ppo_minibatch_step_pop.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, i32, vp, vp, vp, i64, i32, vp, i32, f32,
                                             f32, f32, vp, vp, vp, vp]
    L.pcc_gae_pop.argtypes = [vp, vp, vp, vp, i32, i64, i32, vp, vp, vp, vp]
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    res = {}

    def ok(rc):
        assert rc == 0, rc

    # ---- GAE, stand-alone and per member
    g = torch.Generator().manual_seed(99)
    for name, n in (("gae", 1000), ("gae_pop", K * ROWS)):
        rew, val, last = torch.randn(T, n, generator=g).to(dev), torch.randn(T, n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
        done = (torch.rand(T, n, generator=g) < 0.2).to(torch.uint8).to(dev)
        adv, ret = torch.zeros(T, n, device=dev), torch.zeros(T, n, device=dev)
        if name == "gae":
            ok(L.pcc_gae(p(rew), p(val), p(done), p(last), T, n, 0.99, 0.95, p(adv), p(ret), None))
        else:
            hyper = torch.tensor(HYPER, dtype=torch.float32).to(dev)
            ok(L.pcc_gae_pop(p(rew), p(val), p(done), p(last), T, n, K, p(hyper), p(adv), p(ret), None))
        torch.cuda.synchronize()
        res[name + "/adv"], res[name + "/ret"] = adv.cpu(), ret.cpu()

    for si, (D, h1, h2) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(100 + D)
        key = "%d_%d_%d" % (D, h1, h2)
        n_net = h1 * D + h1 + h2 * h1 + h2 + h2 + 1
        n_params = 2 * n_net + 1
        params = (0.2 * torch.randn(n_params, generator=g)).to(dev)
        n, count = (70000, 66000) if si == 0 else (5000, 4097)

        def batch(n):
            return (torch.randn(n, D, generator=g).to(dev), (0.5 * torch.randn(n, generator=g)).to(dev),
                    (-1.0 + 0.3 * torch.randn(n, generator=g)).to(dev), torch.randn(n, generator=g).to(dev),
                    (2.0 * torch.randn(n, generator=g)).to(dev), torch.randn(n, generator=g).to(dev))
        obs, act, logp, adv, ret, noise = batch(n)
        perm = torch.randperm(n, generator=g).to(dev)
        floats = L.pcc_ppo_scratch_floats(D, h1, h2)
        scratch = torch.empty(floats, device=dev)
        # ---- the gradient alone (lr = 0, no moments), with a permutation and without one
        for name, pm in (("", perm), ("_noperm", None)):
            grad, stats = torch.zeros(n_params, device=dev), torch.zeros(4, device=dev)
            ok(L.pcc_ppo_minibatch_step(p(obs), p(act), p(logp), p(adv), p(ret), p(pm), 7, count, D, h1, h2, p(params), None, None, 1,
                                        0.0, 0.9, 0.999, 1e-5, 0.2, 0.01, p(scratch), p(grad), p(stats), None))
            torch.cuda.synchronize()
            res[key + "/grad" + name], res[key + "/stats" + name] = grad.cpu(), stats.cpu()
        # ---- three optimiser steps
        prm, m, v = params.clone(), torch.zeros(n_params, device=dev), torch.zeros(n_params, device=dev)
        for step in (1, 2, 3):
            ok(L.pcc_ppo_minibatch_step(p(obs), p(act), p(logp), p(adv), p(ret), p(perm), 7 + 100 * step, min(count, 4097), D, h1, h2, p(prm),
                                        p(m), p(v), step, 1e-3, 0.9, 0.999, 1e-5, 0.2, 0.01, p(scratch), None, None, None))
        torch.cuda.synchronize()
        res[key + "/adam_params"], res[key + "/adam_m"], res[key + "/adam_v"] = prm.cpu(), m.cpu(), v.cpu()
        # ---- the forward
        outs = [torch.zeros(n, device=dev) for _ in range(4)]
        ok(L.pcc_policy_act(p(obs), n, D, p(params), h1, h2, p(noise), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None))
        torch.cuda.synchronize()
        for name, t in zip(("mean", "act", "logp", "value"), outs):
            res[key + "/" + name] = t.cpu()
        # ---- the population entry points: K members x ROWS rows
        n = K * ROWS
        stride = (n_params + 63) // 64 * 64
        obs, act, logp, adv, ret, noise = batch(n)
        pp = torch.zeros(K, stride)
        pp[:, :n_params] = 0.2 * torch.randn(K, n_params, generator=g)
        pp = pp.to(dev)
        hyper = torch.tensor(HYPER, dtype=torch.float32).to(dev)
        outs = [torch.zeros(n, device=dev) for _ in range(4)]
        ok(L.pcc_policy_act_pop(p(obs), n, D, p(pp), stride, K, h1, h2, p(noise), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None))
        torch.cuda.synchronize()
        for name, t in zip(("mean", "act", "logp", "value"), outs):
            res[key + "/pop_" + name] = t.cpu()
        perm = torch.stack([k * ROWS + torch.randperm(ROWS, generator=g) for k in range(K)]).to(dev)   # a member's own rows, shuffled
        m, v = torch.zeros(K, stride, device=dev), torch.zeros(K, stride, device=dev)
        grad, stats = torch.zeros(K, stride, device=dev), torch.zeros(K, 4, device=dev)
        scratch = torch.empty(K * floats, device=dev)
        for step in (1, 2):
            ok(L.pcc_ppo_minibatch_step_pop(p(obs), p(act), p(logp), p(adv), p(ret), p(perm), ROWS, 3 * step, 250, D, h1, h2, p(pp), p(m), p(v),
                                            stride, K, p(hyper), step, 0.9, 0.999, 1e-5, p(scratch), p(grad), p(stats), None))
        torch.cuda.synchronize()
        for name, t in zip(("params", "m", "v", "grad", "stats"), (pp, m, v, grad, stats)):
            res[key + "/pop_step_" + name] = t.cpu()
    torch.save(res, out)
    print("wrote", out, len(res), "tensors")


def compare(a, b):
    A, B = torch.load(a), torch.load(b)
    assert sorted(A) == sorted(B)
    bad = [k for k in sorted(A) if not torch.equal(A[k], B[k])]
    for k in sorted(A):
        print(k, "equal" if k not in bad else "DIFFERENT (max |a - b| = %g)" % (A[k] - B[k]).abs().max().item(), "|x| max %g" % A[k].abs().max().item())
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        dump(sys.argv[1], sys.argv[2])
