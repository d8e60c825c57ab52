#!/usr/bin/env python3
"""The PPO kernels' outputs on seeded inputs, one shape per kernel family, straight through the C ABI of ONE build of the
library, into a .pt file -- to compare two builds (GPU box):
   python tools/dump_ppo_outputs.py path/libpcc_sim.so out.pt          for each build, then
   python tools/dump_ppo_outputs.py --compare a.pt b.pt                torch.equal on every tensor
For every shape of SHAPES: the gradient and statistics of a seeded minibatch (pcc_ppo_minibatch_step, lr = 0, with a
permutation; 66 000 samples from row 7 on: ragged last tiles of both 32 and 64 samples, more tiles than workgroups) and
pcc_policy_act's four outputs.  Uses only symbols every build has."""
import ctypes, sys
import torch

SHAPES = [(30, 32, 16), (12, 32, 16),   # ppo_grad_mfma_kernel + policy_act_fixed_kernel
          (36, 32, 16),                 # policy_act_fixed_kernel + the tiled gradient, DP 64
          (30, 16, 8),                  # the generic policy_act_kernel + tiled DP 32
          (45, 48, 24),                 # tiled 64 / (64, 32)
          (120, 64, 64),                # tiled 128 / (64, 64)
          (1, 1, 1)]                    # all padding


def dump(path, out):
    L = ctypes.CDLL(path)
    L.pcc_ppo_scratch_floats.restype = ctypes.c_int
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    L.pcc_policy_act.argtypes = [vp, i64, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.pcc_ppo_minibatch_step.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, vp, vp, vp, i32, f32, f32, f32, f32,
                                         f32, f32, vp, vp, vp, vp]
    dev = torch.device("cuda:0")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    res = {}
    for D, h1, h2 in SHAPES:
        g = torch.Generator().manual_seed(100 + D)
        n_net = h1 * D + h1 + h2 * h1 + h2 + h2 + 1
        params = (0.2 * torch.randn(2 * n_net + 1, generator=g)).to(dev)
        n, count = 70000, 66000
        obs = torch.randn(n, D, generator=g).to(dev)
        act = (0.5 * torch.randn(n, generator=g)).to(dev)
        logp = (-1.0 + 0.3 * torch.randn(n, generator=g)).to(dev)
        adv = torch.randn(n, generator=g).to(dev)
        ret = (2.0 * torch.randn(n, generator=g)).to(dev)
        noise = torch.randn(n, generator=g).to(dev)
        perm = torch.randperm(n, generator=g).to(dev)
        scratch = torch.empty(L.pcc_ppo_scratch_floats(D, h1, h2), device=dev)
        grad, stats = torch.zeros(2 * n_net + 1, device=dev), torch.zeros(4, device=dev)
        rc = L.pcc_ppo_minibatch_step(p(obs), p(act), p(logp), p(adv), p(ret), p(perm), 7, count, D, h1, h2, p(params), None, None, 1,
                                      0.0, 0.9, 0.999, 1e-5, 0.2, 0.01, p(scratch), p(grad), p(stats), None)
        assert rc == 0, rc
        outs = [torch.zeros(n, device=dev) for _ in range(4)]
        rc = L.pcc_policy_act(p(obs), n, D, p(params), h1, h2, p(noise), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        key = "%d_%d_%d" % (D, h1, h2)
        res[key + "/grad"], res[key + "/stats"] = grad.cpu(), stats.cpu()
        for name, t in zip(("mean", "act", "logp", "value"), outs):
            res[key + "/" + name] = t.cpu()
    torch.save(res, out)
    print("wrote", out, sorted(res))


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
