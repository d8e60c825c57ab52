"""Keyed random streams of the learners, the part that needs no GPU (include/pcc_policy.h: pcc_rollout_noise_pop, pcc_sample_order_pop,
pcc_adv_standardise_pop and their stand-alone forms): the C-ABI symbols and their refusals (they come before any
device call), the compiler's resource report of the kernels, what rng="philox" refuses and adds to a checkpoint, and the properties of
the numpy restatement of tests/models/learner_streams_model.py that tests/test_learner_streams.py holds the kernels to: the order is a
permutation at every domain edge, uniform by a chi-square bound, the normals have the moments of a standard normal, the
standardisation is torch's float64 formula."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import learner_streams_model as model   # noqa: E402

from pcc_rl_amd import native, streams   # noqa: E402
from pcc_rl_amd.native import lib   # noqa: E402
from pcc_rl_amd.ppo import PPO, PopulationPPO   # noqa: E402

SYMBOLS = {"pcc_rollout_noise_pop": 8, "pcc_sample_order_pop": 9, "pcc_adv_standardise_scratch_doubles": 3, "pcc_adv_standardise_pop": 8,
           "pcc_rollout_noise": 7, "pcc_sample_order": 7, "pcc_adv_standardise": 7}
# every even-bit domain edge 4^h - 1, 4^h, 4^h + 1 up to 4096
SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096]
KEY = model.key_from_seed(3)
M32 = model.M32


# ------------------------------------------------------------------------------------------------------------- the library
def test_the_symbols_are_exported():
    L = lib()
    for s, n_args in SYMBOLS.items():
        assert s in native.SYMBOLS, s
        assert len(getattr(L, s).argtypes) == n_args and getattr(L, s).restype is ctypes.c_int, s


def test_refusals_need_no_device():
    """Every refusal of the header returns -1 before any device call: the pointers here are never dereferenced on the host."""
    L = lib()
    p = ctypes.c_void_p(4096)   # stands for a device pointer

    def noise(T=4, N=12, K=3, out=p, keys=p):
        return L.pcc_rollout_noise_pop(out, None, T, N, K, keys, 1, None)

    def order(T=4, N=12, K=3, stride=16, out=p, keys=p):
        return L.pcc_sample_order_pop(out, stride, T, N, K, keys, 1, 0, None)

    def stand(T=4, N=12, K=3, adv=p, scratch=p, moments=p, out=p):
        return L.pcc_adv_standardise_pop(adv, T, N, K, scratch, moments, out, None)

    for fn in (noise, order, stand):
        assert fn(T=0) == -1 and fn(T=-3) == -1, fn.__name__
        assert fn(N=0) == -1 and fn(N=13) == -1, fn.__name__            # n_envs % n_members != 0
        assert fn(K=0) == -1 and fn(K=1025, N=1025) == -1, fn.__name__
        assert fn(N=3 * 2 ** 31, K=3) == -1, fn.__name__                # n_m < 2^31
    assert noise(out=None) == -1 and noise(keys=None) == -1
    assert order(out=None) == -1 and order(keys=None) == -1
    assert order(stride=15) == -1 and order(stride=-1) == -1            # perm_stride < T * n_m = 16
    for name in ("adv", "scratch", "moments", "out"):
        assert stand(**{name: None}) == -1, name
    assert L.pcc_rollout_noise(None, None, 4, 12, 1, 1, None) == -1 and L.pcc_rollout_noise(p, None, 0, 12, 1, 1, None) == -1
    assert L.pcc_sample_order(None, 4, 12, 1, 1, 0, None) == -1 and L.pcc_sample_order(p, 4, 0, 1, 1, 0, None) == -1
    assert L.pcc_adv_standardise(None, 4, 12, p, p, p, None) == -1 and L.pcc_adv_standardise(p, 0, 12, p, p, p, None) == -1
    # the scratch: two passes x the member's workgroups of 256 lanes
    assert L.pcc_adv_standardise_scratch_doubles(64, 65536, 8) == 2 * 8 * 32
    assert L.pcc_adv_standardise_scratch_doubles(1, 257, 1) == 4 and L.pcc_adv_standardise_scratch_doubles(1, 3, 3) == 6
    assert L.pcc_adv_standardise_scratch_doubles(0, 12, 3) == -1 and L.pcc_adv_standardise_scratch_doubles(4, 13, 3) == -1


def test_the_kernels_are_in_the_resource_report(tmp_path):
    """A build into a temporary file: the five kernels of pcc_streams.hip use no scratch and spill no vector register; none is a
    `_pop_kernel` twin (tests/test_population_cpu.py lists every kernel of that name)."""
    from pcc_rl_amd import build as pbuild
    out = str(tmp_path / "libpcc_sim_streams.so")
    pbuild.build_library(force=True, out=out)
    res = json.load(open(out + ".resources.json"))
    names = ["rollout_noise_kernel", "sample_order_kernel", "adv_sum_kernel<0>", "adv_sum_kernel<1>", "adv_apply_kernel"]
    for name in names:
        assert name in res, (name, sorted(res))
        r = res[name]
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["lds"] <= 64 * 1024, (name, r)
    assert not [n for n in res if "_pop_kernel" in n]
    assert "pcc_streams.hip" in pbuild.UNITS


# --------------------------------------------------------------------------------------------------------------- the model
def test_reference_philox_known_answers():
    # Random123 kat_vectors, philox4x32-10 (tests/test_pbt_cpu.py holds its own copy to the same)
    kats = [((0, 0, 0, 0), (0, 0), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
            ((M32,) * 4, (M32,) * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kats:
        assert model.philox4x32_10(ctr, key) == want
        assert model.philox_array(*ctr, key[0] | (key[1] << 32)).tolist() == want     # the array form is the integer form
    w = model.noise_words(KEY, 7, 3, 10)
    for t, e in ((0, 0), (2, 9), (1, 6)):
        assert int(w[t, e]) == model.philox4x32_10((e >> 2, t, 7, model.TAG_NOISE), (KEY & M32, KEY >> 32))[e & 3]


def test_keys_from_seeds():
    assert [streams.key_from_seed(s) for s in (0, 1, 2, 12345, 2 ** 63)] == [model.key_from_seed(s) for s in (0, 1, 2, 12345, 2 ** 63)]
    assert model.key_from_seed(0) == 0xE220A8397B1DCDAF     # splitmix64's first output from state 0
    keys = [model.key_from_seed(s) for s in range(64)]
    assert len(set(keys)) == 64 and all(0 <= k < 2 ** 64 for k in keys)
    # neighbouring seeds differ in about half of the key's bits: 64 fair bits are 32 +- 4, five standard deviations either way
    assert all(12 <= bin(a ^ b).count("1") <= 52 for a, b in zip(keys, keys[1:]))


@pytest.mark.parametrize("n", SIZES)
def test_the_order_is_a_permutation(n):
    for it, ep in ((1, 0), (1, 3), (2, 0)):
        p, walks = model.order_local(KEY, it, ep, n, with_walks=True)
        assert sorted(p.tolist()) == list(range(n)), (n, it, ep)
        assert 4 ** model.half_bits(n) >= n and (model.half_bits(n) == 0 or 4 ** (model.half_bits(n) - 1) < n)
        # the walks from [0, n) are disjoint pieces of the cycles: together they visit every value at most once, so their mean length is
        # at most 4^h / n < 4, and none is longer than the 4^h - n values outside [0, n) plus its end
        assert walks.sum() <= 4 ** model.half_bits(n) and walks.mean() < 4.0 and walks.max() <= 4 ** model.half_bits(n) - n + 1


def test_the_order_differs_by_epoch_iteration_and_key():
    n = 1025
    base = model.order_local(KEY, 1, 0, n)
    assert np.array_equal(base, model.order_local(KEY, 1, 0, n))
    for other in (model.order_local(KEY, 1, 1, n), model.order_local(KEY, 2, 0, n), model.order_local(model.key_from_seed(4), 1, 0, n)):
        assert not np.array_equal(base, other)
        assert (base == other).mean() < 0.02     # (two random permutations agree at about one position)


def test_the_order_does_not_change_with_the_population():
    """Member 1 of three and the same key alone: the same local permutation, as global indices of its own columns."""
    T, n_m = 7, 5
    keys = [model.key_from_seed(s) for s in (4, 5, 6)]
    alone = model.order_global(keys[1:2], 3, 2, T, n_m)[0]
    pop = model.order_global(keys, 3, 2, T, 3 * n_m)[1]
    local = lambda g, N, m: (g // N) * n_m + (g % N - m * n_m)
    assert np.array_equal(local(alone, n_m, 0), local(pop, 3 * n_m, 1))
    assert np.array_equal(local(alone, n_m, 0), model.order_local(keys[1], 3, 2, T * n_m))
    assert ((pop % (3 * n_m)) // n_m == 1).all()             # inside the member's columns
    again = model.order_global(keys[::-1], 3, 2, T, 3 * n_m)[1]     # ... and in another slot beside other members
    assert np.array_equal(pop, again)


def test_the_order_is_uniform():
    """n = 4096, 48 keys, the 16 x 16 table of (position bucket, value bucket): chi-square below the 0.999 quantile of chi2(225), 296.3
    by Wilson-Hilferty.  (numpy's own permutation gave 216.6 on this table.)"""
    n, table = 4096, np.zeros((16, 16))
    for s in range(48):
        p = model.order_local(model.key_from_seed(s), 1, 0, n)
        np.add.at(table, (np.arange(n) // 256, p // 256), 1)
    expected = 48 * n / 256.0
    chi2 = float(((table - expected) ** 2 / expected).sum())
    print("chi-square of the 16 x 16 table: %.1f" % chi2)
    wilson_hilferty = 225 * (1 - 2 / (9 * 225) + 3.0902 * np.sqrt(2 / (9 * 225))) ** 3
    assert abs(wilson_hilferty - 296.3) < 0.1
    assert chi2 < 296.3


def test_the_normals_have_standard_moments():
    z = model.noise64(model.key_from_seed(0), 1, 64, 16384)     # 2^20 draws
    assert z.shape == (64, 16384) and np.isfinite(z).all()
    n = z.size
    print("mean %.3e  variance %.6f  max |z| %.3f" % (z.mean(), z.var(), np.abs(z).max()))
    assert abs(z.mean()) < 5.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)
    assert np.abs(z).max() <= np.sqrt(64 * np.log(2.0))
    # the two normals of a pair and the two pairs of a block are uncorrelated
    assert abs(np.mean(z[:, 0::4] * z[:, 1::4])) < 5.0 / np.sqrt(n / 4) and abs(np.mean(z[:, 0::4] * z[:, 2::4])) < 5.0 / np.sqrt(n / 4)
    # a member's values are those of its key alone, whatever n_m rounds up to
    assert np.array_equal(model.noise64(KEY, 2, 3, 257)[:, :10], model.noise64(KEY, 2, 3, 10))


def test_sincos_reduction():
    b = np.array([0, 1, 2 ** 29, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31, 3 * 2 ** 30, 2 ** 32 - 1, 123456789], dtype=np.uint64)
    s, c = model._sincos_2pi(b)
    assert (s[0], c[0]) == (0.0, 1.0) and (s[4], c[4]) == (1.0, 0.0) and (s[6], c[6]) == (0.0, -1.0) and (s[7], c[7]) == (-1.0, 0.0)
    ang = 2.0 * np.pi * b.astype(np.float64) / 2.0 ** 32
    assert np.allclose(s, np.sin(ang), rtol=0, atol=1e-15) and np.allclose(c, np.cos(ang), rtol=0, atol=1e-15)
    assert c[5] == -s[1] and abs(s[1] / (2.0 * np.pi / 2.0 ** 32) - 1.0) < 1e-15      # exact symmetry next to a zero


@pytest.mark.parametrize("T,K,n_m", [(6, 3, 37), (12, 3, 257), (1, 1, 1000), (3, 2, 70000 // 3)])
def test_standardisation_is_torchs_formula(T, K, n_m):
    g = torch.Generator().manual_seed(T + n_m)
    adv = (torch.randn(T, K * n_m, generator=g) * torch.tensor([1.0, 10.0, 0.1])[:K].repeat_interleave(n_m) + 3.0).numpy()
    got, moments = model.standardise(adv, K)
    for m in range(K):
        a = torch.from_numpy(adv[:, m * n_m:(m + 1) * n_m]).double().reshape(-1)
        want = ((a - a.mean()) / (a.std() + 1e-8)).reshape(T, n_m).numpy()
        want32 = want.astype(np.float32)
        assert (np.abs(got[:, m * n_m:(m + 1) * n_m].astype(np.float64) - want) <= np.spacing(np.abs(want32))).all(), m
        assert abs(moments[m, 0] - float(a.mean())) <= 1e-14 * abs(float(a.mean())) + 1e-300
        assert abs(moments[m, 1] - float(a.var())) <= 1e-13 * float(a.var())


def test_standardisation_edges():
    out, mom = model.standardise(np.full((5, 12), 2.5, dtype=np.float32), 3)     # constant: all 0
    assert (out == 0.0).all() and (mom[:, 0] == 2.5).all() and (mom[:, 1] == 0.0).all()
    out, mom = model.standardise(np.array([[1.0, 2.0, 3.0]], dtype=np.float32), 3)     # one sample per member: NaN, as torch's std
    assert np.isnan(out).all() and np.isnan(mom[:, 1]).all() and mom[:, 0].tolist() == [1.0, 2.0, 3.0]


# ------------------------------------------------------------------------------------------------------------ the trainers
class _Env(object):   # what the constructors' argument checks look at, without a simulator behind it
    obs_dim, device, n_senders, n_envs = 30, "cuda:0", 1, 12


class _CpuEnv(_Env):
    device = "cpu"


class _TwoSenders(_Env):
    n_senders = 2


def test_constructors_refuse():
    for cls, args in ((PPO, ()), (PopulationPPO, (3,))):
        with pytest.raises(ValueError, match='rng = \'cuda\' \\("torch" or "philox"\\)'):
            cls(_Env(), *args, rng="cuda")
    for env, kw in ((_CpuEnv(), {}), (_TwoSenders(), {}), (_Env(), {"arch": (32, 16, 8)}), (_Env(), {"arch": (32,)})):
        with pytest.raises(ValueError, match="needs the fused rollout"):
            PPO(env, rng="philox", **kw)
    with pytest.raises(ValueError, match="needs the fused update"):
        PPO(_Env(), rng="philox", fused_update=False)
    # PopulationPPO on anything it already refuses: its own messages, with or without the option
    with pytest.raises(ValueError, match="do not divide"):
        PopulationPPO(_Env(), 5, rng="philox")
    with pytest.raises(ValueError, match="two hidden layers"):
        PopulationPPO(_Env(), 3, arch=(32, 16, 8), rng="philox")
    with pytest.raises(ValueError, match="BatchedNetworkEnv"):
        PopulationPPO(_Env(), 3, rng="philox")
    with pytest.raises(ValueError, match="GPU device"):
        streams.LearnerStreams([0], 12, device="cpu")
    with pytest.raises(ValueError, match="do not divide"):
        streams.LearnerStreams([0, 1, 2, 3, 4], 12, device="cuda:0")


class _Streams(object):   # LearnerStreams' two checkpoint methods, without a device
    def __init__(self, keys):
        self.keys = list(keys)

    def state_dict(self):
        return {"keys": list(self.keys), "n_envs": 12}

    def load_state_dict(self, sd):
        self.keys = list(sd["keys"])


class _Snap(_CpuEnv):
    restored = None

    def snapshot(self):
        return "snapshot"

    def restore(self, s):
        self.restored = s


def _trainer(rng, keys=(1, 2)):
    """A PPO object with the fields _common_state / _restore read and nothing else: no device, no library."""
    t = PPO.__new__(PPO)
    t.env, t.obs, t.rng, t.iteration = _Snap(), torch.zeros(12, 30), rng, 0
    t.normalize_obs = t.track_episodes = t.normalize_reward = t.diagnostics = False
    t.target_kl, t.streams = None, _Streams(keys) if rng == "philox" else None
    t._load_params = lambda sd: None
    return t


def test_checkpoint_fields():
    a = _trainer("philox", keys=(model.key_from_seed(4), 2 ** 64 - 1))
    a.iteration = 5
    sd = a._common_state()
    assert sd["rng"] == "philox" and sd["iteration"] == 5 and sd["streams"] == {"keys": [model.key_from_seed(4), 2 ** 64 - 1], "n_envs": 12}
    plain = _trainer("torch")._common_state()
    assert not {"rng", "streams", "iteration"} & set(plain)       # the default's checkpoint has the keys it had
    assert set(sd) - set(plain) == {"rng", "streams", "iteration"}
    b = _trainer("philox", keys=(0, 0))
    b._restore(sd)
    assert b.iteration == 5 and b.streams.keys == a.streams.keys and b.env.restored == "snapshot"
    for mine, theirs in (("torch", sd), ("philox", plain)):
        other = _trainer(mine)
        with pytest.raises(ValueError, match="written with rng="):
            other._restore(theirs)
        assert other.env.restored is None      # refused before anything is restored
