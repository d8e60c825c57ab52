"""Population-based training's step between generations, the part that needs no GPU: the C-ABI symbol pcc_pbt_evolve
(include/pcc_policy.h), its refusals (they come before any device call), the compiler's resource report of pbt_evolve_kernel, and this
file's own numpy restatement of the contract -- evolve_reference, with its own Philox4x32-10 and an explicit O(K^2) ranking --
which tests/test_pbt.py holds the kernel against, bit for bit."""
import ctypes
import json

import numpy as np
import pytest

from pcc_rl_amd import native
from pcc_rl_amd.native import lib

PAD = 7.0   # what the padding of every [members][param_stride] block holds before a call -- and after it
INF = float("inf")
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------ the reference
def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011) on Python integers: four counter words, two key words -> four words."""
    c0, c1, c2, c3 = (int(x) & M32 for x in ctr)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0, p1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def ranks(score):
    """rank[m] = the number of members better than m: a is better than b when exactly one of the two scores is NaN and a's is
    not; else when neither is NaN, the scores differ and a's is larger; else when a < b.  The whole K x K table, no sort."""
    s = np.asarray(score, dtype=np.float64)
    K = s.shape[0]
    nan = np.isnan(s)
    a, b = np.meshgrid(np.arange(K), np.arange(K), indexing="ij")       # better[a][b]: a is better than b
    with np.errstate(invalid="ignore"):
        differ = ~nan[a] & ~nan[b] & (s[a] != s[b])
        better = np.where(nan[a] != nan[b], ~nan[a], np.where(differ, s[a] > s[b], a < b))
    better[np.arange(K), np.arange(K)] = False
    return better.sum(axis=0).astype(np.int32)


def evolve_reference(score, n_cut, params, adam_m, adam_v, n_params, hyper, explore, seed, generation):
    """The contract of pcc_pbt_evolve on numpy arrays ([K][stride] float32 blocks, [K][8] hyper, [8][4] explore): returns new
    (params, adam_m, adam_v, hyper, parent, rank); the inputs are left as they are."""
    K = len(score)
    rank = ranks(score)
    n_valid = int((~np.isnan(np.asarray(score, dtype=np.float64))).sum())
    n_src = min(n_cut, n_valid)
    by_rank = np.empty(K, dtype=np.int64)
    by_rank[rank] = np.arange(K)
    out = [np.array(x, dtype=np.float32, copy=True) for x in (params, adam_m, adam_v, hyper)]
    old = [np.asarray(x, dtype=np.float32) for x in (params, adam_m, adam_v, hyper)]
    explore = np.asarray(explore, dtype=np.float32)
    parent = np.arange(K, dtype=np.int32)
    for m in range(K):
        if not (n_src > 0 and rank[m] >= K - n_cut):
            continue
        w = philox4x32_10((m, generation, 0, 0), (seed & M32, (seed >> 32) & M32))
        p = int(by_rank[(w[0] * n_src) >> 32])
        for new, was in zip(out[:3], old[:3]):
            new[m, :n_params] = was[p, :n_params]
        for c in range(8):
            f = explore[c, 1] if (w[1] >> c) & 1 else explore[c, 0]
            out[3][m, c] = np.fmin(np.fmax(np.float32(old[3][p, c] * f), explore[c, 2]), explore[c, 3])
        parent[m] = p
    return out[0], out[1], out[2], out[3], parent, rank


# ------------------------------------------------------------------------------------------------- the cases of both files
SHAPES = [(1, 70, 128), (2, 3075, 3136), (5, 3075, 3136), (8, 3075, 3136), (7, 257, 320), (33, 1, 64), (3, 24963, 25024), (1024, 70, 128)]
SCORE_KINDS = ["distinct", "equal", "ties", "inf", "third_nan", "all_nan", "few_valid"]
# column 0: two factors, no bounds; column 2: bounds that clamp N(0, 1) values from both sides; the rest inherit
EXPLORE = [[0.8, 1.2, -INF, INF], [1.0, 1.0, -INF, INF], [0.5, 2.0, -0.75, 0.5]] + [[1.0, 1.0, -INF, INF]] * 5


def n_cuts(K):
    return sorted(c for c in {0, 1, K // 4, K // 2} if 2 * c <= K)


def make_scores(kind, K, n_cut, rng):
    s = rng.standard_normal(K)
    if kind == "equal":
        s[:] = 1.5
    elif kind == "ties":               # pairs of equal scores, and +0.0 next to -0.0
        s = rng.permutation(np.repeat(rng.standard_normal(K // 2 + 1), 2)[:K])
        if K >= 2:
            s[0], s[K - 1] = 0.0, -0.0
    elif kind == "inf":
        s[0] = INF
        s[K - 1] = -INF
        if K >= 5:
            s[2], s[3] = INF, -INF
    elif kind == "third_nan":
        s[rng.choice(K, max(1, K // 3), replace=False)] = np.nan
        s[np.nonzero(np.isnan(s))[0][::2]] = np.copysign(np.nan, -1.0)   # (either sign of NaN)
    elif kind == "all_nan":
        s[:] = np.nan
    elif kind == "few_valid":          # fewer numbers than n_cut: the sources are those alone
        keep = rng.choice(K, n_cut // 2, replace=False)
        t = np.full(K, np.nan)
        t[keep] = s[keep]
        s = t
    return s


def make_case(K, n_params, stride, seed):
    """[K][stride] blocks with PAD in the padding -- normal floats, and raw random bits in adam_v (NaN payloads, denormals, signed
    zeros must come through a copy) -- and a [K][8] hyper block of normal floats."""
    rng = np.random.default_rng(seed)
    blocks = []
    for i in range(3):
        b = np.full((K, stride), PAD, dtype=np.float32)
        if i < 2:
            b[:, :n_params] = rng.standard_normal((K, n_params)).astype(np.float32)
        else:
            b[:, :n_params] = rng.integers(0, 2 ** 32, (K, n_params), dtype=np.uint32).view(np.float32)
        blocks.append(b)
    hyper = rng.standard_normal((K, 8)).astype(np.float32)
    return blocks[0], blocks[1], blocks[2], hyper


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------- tests
def test_the_symbol_is_exported():
    L = lib()
    assert "pcc_pbt_evolve" in native.SYMBOLS
    assert hasattr(L, "pcc_pbt_evolve")
    assert len(L.pcc_pbt_evolve.argtypes) == 15 and L.pcc_pbt_evolve.restype is ctypes.c_int


def test_refusals_need_no_device():
    """Every refusal of the header returns -1 before any device call: the pointers here are never dereferenced on the host, and
    nothing on this path needs a GPU."""
    L = lib()
    p = ctypes.c_void_p(4096)   # stands for a device pointer

    def call(K=8, cut=2, stride=3136, n=3075, score=p, params=p, m=p, v=p, hyper=p, explore=p):
        return L.pcc_pbt_evolve(score, K, cut, params, m, v, stride, n, hyper, explore, 0, 0, None, None, None)

    for K in (0, -1, 1025):
        assert call(K=K, cut=0) == -1, K
    assert call(cut=-1) == -1
    assert call(cut=5) == -1 and call(K=1, cut=1) == -1 and call(K=7, cut=4) == -1     # 2 n_cut > n_members
    assert call(K=1024, cut=513) == -1
    for stride in (3075, 3136 + 32, 3137):
        assert call(stride=stride) == -1, stride
    assert call(n=0) == -1 and call(n=-5) == -1 and call(n=3137) == -1
    assert call(stride=0, n=1) == -1
    for name in ("score", "params", "m", "v", "hyper", "explore"):
        assert call(**{name: None}) == -1, name


def test_the_kernel_is_in_the_resource_report(tmp_path):
    """A build into a temporary file: pbt_evolve_kernel uses no scratch, spills no vector register and stays far below a compute
    unit's LDS; it is no `_pop_kernel` (tests/test_population_cpu.py lists every kernel of that name)."""
    from pcc_rl_amd import build as pbuild
    out = str(tmp_path / "libpcc_sim_pbt.so")
    pbuild.build_library(force=True, out=out)
    res = json.load(open(out + ".resources.json"))
    assert "pbt_evolve_kernel" in res, sorted(res)
    r = res["pbt_evolve_kernel"]
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["lds"] <= 64 * 1024, r
    assert not [n for n in res if "pbt" in n and "_pop_kernel" in n]
    assert "pcc_pbt.hip" in pbuild.UNITS


def test_reference_philox_known_answers():
    # Random123 kat_vectors, philox4x32-10 (tests/test_oracle_golden.py holds the oracle's to the same)
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert philox4x32_10([M32] * 4, [M32] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_reference_ranking():
    assert ranks([3.0, 1.0, 2.0, 0.0]).tolist() == [0, 2, 1, 3]
    assert ranks([1.5] * 6).tolist() == list(range(6))                       # all equal: the lowest index first
    assert ranks([0.0, -0.0, 0.0]).tolist() == [0, 1, 2]                     # +0.0 == -0.0: by index
    assert ranks([np.nan, 1.0, np.nan, -INF, INF]).tolist() == [3, 1, 4, 2, 0]   # NaN last, among themselves by index
    assert ranks([np.nan] * 3).tolist() == [0, 1, 2]
    rng = np.random.default_rng(0)
    for kind in SCORE_KINDS:
        for K in (1, 2, 5, 33, 1024):
            for cut in n_cuts(K):
                r = ranks(make_scores(kind, K, cut, rng))
                assert sorted(r.tolist()) == list(range(K)), (kind, K)       # a permutation


@pytest.mark.parametrize("kind", SCORE_KINDS)
def test_reference_properties(kind):
    """Replaced members and sources are disjoint, every parent of a replaced member has rank < n_src, rows that are not replaced
    and all padding stay as they were, a {1, 1, -inf, +inf} column is inherited exactly."""
    rng = np.random.default_rng(5)
    for K, n, stride in [(2, 5, 64), (5, 70, 128), (33, 1, 64), (1024, 3, 64)]:
        P, M, V, H = make_case(K, n, stride, K)
        for cut in n_cuts(K):
            s = make_scores(kind, K, cut, rng)
            p2, m2, v2, h2, parent, rank = evolve_reference(s, cut, P, M, V, n, H, EXPLORE, 11, 3)
            n_src = min(cut, int((~np.isnan(s)).sum()))
            replaced = np.nonzero(parent != np.arange(K))[0]
            assert len(replaced) == (cut if n_src > 0 else 0)
            assert not set(replaced.tolist()) & set(parent[replaced].tolist())
            assert (rank[parent[replaced]] < n_src).all() and (rank[replaced] >= K - cut).all()
            assert not np.isnan(s[parent[replaced]]).any()
            keep = parent == np.arange(K)
            for new, was in ((p2, P), (m2, M), (v2, V), (h2, H)):
                assert np.array_equal(bits(new[keep]), bits(was[keep]))
            for new, was in ((p2, P), (m2, M), (v2, V)):
                assert np.array_equal(bits(new[replaced, :n]), bits(was[parent[replaced], :n]))
                assert (new[:, n:] == PAD).all()
            assert np.array_equal(bits(h2[replaced][:, [1, 3, 4, 5, 6, 7]]), bits(H[parent[replaced]][:, [1, 3, 4, 5, 6, 7]]))
            ratio = np.round(h2[replaced, 0].astype(np.float64) / H[parent[replaced], 0], 3)
            assert np.isin(ratio, [0.8, 1.2]).all()
            assert (h2[replaced, 2] >= -0.75).all() and (h2[replaced, 2] <= 0.5).all()
            if K == 1024 and cut == 256 and kind == "distinct":
                assert (h2[replaced, 2] == -0.75).any() and (h2[replaced, 2] == 0.5).any()     # the bounds clamp from both sides
                assert {0.8, 1.2} == set(ratio.tolist())
                assert len(set(parent[replaced].tolist())) > 100                               # many different sources


DRAWS = [(1, 0), (1, 1), (2, 0)]   # (seed, generation): tests/test_pbt.py runs the same three on the GPU


def test_another_seed_or_generation_draws_other_parents():
    K, cut = 1024, 256
    P, M, V, H = make_case(K, 70, 128, 1)
    s = make_scores("distinct", K, cut, np.random.default_rng(1))
    parents = [evolve_reference(s, cut, P, M, V, 70, H, EXPLORE, seed, gen)[4] for seed, gen in DRAWS]
    assert not np.array_equal(parents[0], parents[1]) and not np.array_equal(parents[0], parents[2])
    assert not np.array_equal(parents[1], parents[2])
    again = evolve_reference(s, cut, P, M, V, 70, H, EXPLORE, *DRAWS[0])[4]
    assert np.array_equal(again, parents[0])
    big = evolve_reference(s, cut, P, M, V, 70, H, EXPLORE, (5 << 32) | 1, 0)[4]    # the high word of the seed is the second key word
    assert not np.array_equal(big, parents[0])


def test_explore_matrix_and_frac():
    from pcc_rl_amd.ppo import PopulationPPO, explore_matrix
    rows = explore_matrix()
    assert rows[0] == [0.8, 1.2, -INF, INF] and rows[2] == [0.8, 1.2, -INF, INF]
    assert all(r == [1.0, 1.0, -INF, INF] for i, r in enumerate(rows) if i not in (0, 2)) and len(rows) == 8
    rows = explore_matrix((0.5, 2.0), ("gamma",), {"gamma": (0.9, 0.999), "lr": (1e-5, 1e-2)})
    assert rows[3] == [0.5, 2.0, 0.9, 0.999] and rows[0] == [1.0, 1.0, 1e-5, 1e-2] and rows[2] == [1.0, 1.0, -INF, INF]
    with pytest.raises(ValueError, match="no hyper-parameter"):
        explore_matrix(explore=("momentum",))
    with pytest.raises(ValueError, match="no hyper-parameter"):
        explore_matrix(bounds={"momentum": (0, 1)})
    for frac in (0.6, -0.01, float("nan")):     # (refused before anything of the population is touched)
        with pytest.raises(ValueError, match="frac"):
            PopulationPPO.evolve(object(), [1.0, 2.0], frac=frac)
    assert callable(PopulationPPO.hypers)
