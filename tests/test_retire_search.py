"""The boundary searches and the near-group repairs of the retire half (pcc-rl_amd/csrc/pcc_retire_env.h: search_many<4, G>,
search_boundary<G>, fix_drop_boundary_g<G> with near_window_g / gmin_key / fix_drop_window, drop_hop1_candidate_g<G>) held to linear
scans: the harness kernels of tests/kernels/retire_search_harness.hip run them, unchanged, at 8 and 16 lanes on the case tables of
tests/models/boundary_cases.py, and every index, flag, time, latency and ring record is compared with the reference as integers
or int64 views: there is no tolerance anywhere.  Every lane of a group writes what it got and all of them must agree; the outputs
are prefilled with 0xFFFFFFFF / NaN.  What the tables cover -- every gallop distance above and below the predicted window, every
combination of the four searches of a group missing, near windows of every size 1 .. 2 G + 4 at h, at tail and away from both, b
at every place of its group -- is proved on the CPU, from the inputs alone, in tests/test_boundary_cases_cpu.py.

The harness is a separate compilation of the same source: it holds the algorithm to the scans at inputs the simulator rarely or
never produces; it cannot vouch for the machine code of the six product kernels the header is compiled into -- the simulator's
parity tests hold that to the oracle.

Measured on an MI355X: the 11 tests of this file take 4.7 s together, of which 2.5 s build the tables and their references on the
CPU (once per session, shared by the tests); the slowest test is 0.6 s.  The launches are 2 500 to 16 409 groups each."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import pcc_rl_amd
from pcc_rl_amd import build as pbuild

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import boundary_cases as bc   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIP_ERROR_INVALID_VALUE = 1
P, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


@pytest.fixture(scope="module")
def harness():
    L = ctypes.CDLL(pbuild.build_search_harness())   # (a tree built the usual way has it: this compiles only when it is missing or stale)
    for name, n_in, n_out in (("pcc_test_search_many", 7, 4), ("pcc_test_search_boundary", 6, 1), ("pcc_test_fix_drop_boundary", 7, 4),
                              ("pcc_test_drop_hop1_candidate", 6, 2)):
        f = getattr(L, name)
        f.restype = I32
        f.argtypes = [P, ctypes.c_uint64] + [P] * n_in + [I64, I32] + [P] * n_out + [P]
    return L


def u32(a):
    return torch.as_tensor(np.ascontiguousarray(a).astype(np.uint32).view(np.int32), device=DEV)


def f64(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def call(fn, arena, ins, n, lanes, outs):
    rc = fn(arena.data_ptr(), arena.shape[0], *[x.data_ptr() for x in ins], n, lanes, *[x.data_ptr() for x in outs],
            torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    assert rc == 0, "HIP error %d" % rc
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in outs]


def out_u32(*shape):
    return torch.full(shape, -1, dtype=torch.int32, device=DEV)     # 0xFFFFFFFF


def out_f64(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def one_value_per_group(a, what):
    """(cases, lanes, ...) -> (cases, ...): every lane of a group returned the same bits"""
    a = a.view(np.int64) if a.dtype == np.float64 else a
    assert (a == a[:, :1]).all(), "%s: the lanes of a group differ, first at case %d" % (what, int(np.argwhere(a != a[:, :1])[0][0]))
    return a[:, 0]


def search_many(L, arena, off, mask, lo0, hi0, add, hint, end, lanes):
    """-> b (uint32 as int64), clean (bool), t, lat (int64 views), each (cases, 4), after checking that the lanes agree"""
    n = len(end)
    outs = [out_u32(n, lanes, 4), torch.full((n, lanes, 4), 255, dtype=torch.uint8, device=DEV), out_f64(n, lanes, 4), out_f64(n, lanes, 4)]
    b, clean, t, lat = call(L.pcc_test_search_many, arena, [u32(off), u32(mask), u32(lo0), u32(hi0), f64(add), u32(hint), f64(end)], n, lanes, outs)
    b = one_value_per_group(b.view(np.uint32).astype(np.int64), "b")
    clean = one_value_per_group(clean.astype(np.int64), "clean")
    assert ((clean == 0) | (clean == 1)).all()
    return b, clean == 1, one_value_per_group(t, "t"), one_value_per_group(lat, "lat")


def search_boundary(L, arena, off, mask, lo, hi, add, end, lanes):
    n = len(end)
    (idx,) = call(L.pcc_test_search_boundary, arena, [u32(off), u32(mask), u32(lo), u32(hi), f64(add), f64(end)], n, lanes, [out_u32(n, lanes)])
    return one_value_per_group(idx.view(np.uint32).astype(np.int64), "index")


def fix_drop(L, arena, off, mask, h, tail, b, dl, end, lanes):
    """-> p, cand_idx (int64), cand_t, cand_lat (int64 views); the arena is rewritten"""
    n = len(end)
    outs = [out_u32(n, lanes), out_u32(n, lanes), out_f64(n, lanes), out_f64(n, lanes)]
    p, ci, ct, cl = call(L.pcc_test_fix_drop_boundary, arena, [u32(off), u32(mask), u32(h), u32(tail), u32(b), f64(dl), f64(end)], n, lanes, outs)
    return (one_value_per_group(p.view(np.uint32).astype(np.int64), "p"), one_value_per_group(ci.view(np.uint32).astype(np.int64), "cand_idx"),
            one_value_per_group(ct, "cand_t"), one_value_per_group(cl, "cand_lat"))


def hop1(L, arena, off, mask, h, tail, c, end, lanes):
    n = len(end)
    t, lat = call(L.pcc_test_drop_hop1_candidate, arena, [u32(off), u32(mask), u32(h), u32(tail), u32(c), f64(end)], n, lanes, [out_f64(n, lanes), out_f64(n, lanes)])
    return one_value_per_group(t, "hop-1 t"), one_value_per_group(lat, "hop-1 lat")


# ---------------------------------------------------------------------------------------------- the searches, accepted-like rings
@pytest.fixture(scope="module")
def accepted():
    rings, tab = bc.accepted_rings(), bc.search_table()
    ring = tab["ring"]
    return {"arena": torch.as_tensor(bc.arena_of(rings), device=DEV), "off": np.array([r.off for r in rings])[ring],
            "mask": np.array([r.mask for r in rings])[ring]}


@pytest.mark.parametrize("lanes", [8, 16])
def test_search_many_equals_the_linear_scan(harness, accepted, lanes):
    """b, clean, and ring[b] where b < hi0, of all four searches of every group: hits next to every kind of miss in one wavefront"""
    tab = bc.search_table()
    want_b, want_clean, want_t, want_lat = bc.search_reference()
    b, clean, t, lat = search_many(harness, accepted["arena"], accepted["off"], accepted["mask"], tab["lo0"], tab["hi0"], tab["add"], tab["hint"], tab["end"], lanes)
    bad = np.argwhere(b != want_b)
    assert bad.size == 0, [(int(c), int(k), int(b[c, k]), int(want_b[c, k]), int(tab["lo0"][c, k]), int(tab["hi0"][c, k]), int(tab["hint"][c, k])) for c, k in bad[:8]]
    assert np.array_equal(clean, want_clean)
    has = want_b < tab["hi0"]
    assert has.sum() > 5000
    bad = np.argwhere(has & ((t != bits(want_t)) | (lat != bits(want_lat))))
    assert bad.size == 0, [(int(c), int(k), int(b[c, k]), int(tab["lo0"][c, k]), int(tab["hint"][c, k])) for c, k in bad[:8]]


@pytest.mark.parametrize("lanes", [8, 16])
def test_search_boundary_equals_the_linear_scan(harness, accepted, lanes):
    tab = bc.search_table()
    flat = lambda a: np.ascontiguousarray(a).reshape(-1)
    idx = search_boundary(harness, accepted["arena"], flat(accepted["off"]), flat(accepted["mask"]), flat(tab["lo0"]), flat(tab["hi0"]), flat(tab["add"]),
                          np.repeat(tab["end"], 4), lanes)
    want = flat(bc.search_reference()[0])
    bad = np.flatnonzero(idx != want)
    assert bad.size == 0, [(int(i), int(idx[i]), int(want[i]), int(flat(tab["lo0"])[i]), int(flat(tab["hi0"])[i])) for i in bad[:8]]


# ---------------------------------------------------------------------------------------------- dropped-like rings: the whole flow
def region_arena(regions):
    a = np.empty((sum(g.size for g in regions), 2))
    for g in regions:
        a[g.off:g.off + g.size, 0] = g.t
        a[g.off:g.off + g.size, 1] = g.lat
    return a


def exact_partition(t, mask, lo, hi, b, add, end):
    return all(t[k & mask] + add < end for k in range(lo, b)) and not any(t[k & mask] + add < end for k in range(b, hi))


@pytest.mark.parametrize("lanes", [8, 16])
def test_dropped_ring_flow_gives_what_the_caller_relies_on(harness, lanes):
    """search_many on rings of tie groups; where the drop boundary is not clean the repair, then -- as retire_env does --
    search_boundary from p on and the hop-1 candidate.  The searches may be off inside one near group and say so (`clean`);
    after the repair nothing is."""
    regs = bc.flow_table()
    host = region_arena(regs)
    arena = torch.as_tensor(host, device=DEV)
    col = lambda f: np.array([f(g) for g in regs])
    off, mask, h, tail, dl, end = col(lambda g: g.off), col(lambda g: g.mask), col(lambda g: g.h), col(lambda g: g.tail), col(lambda g: g.dl), col(lambda g: g.end)
    four = lambda a: np.repeat(a[:, None], 4, axis=1)
    add = np.stack([dl, 0 * dl, dl, 0 * dl], axis=1)
    b, clean, t, lat = search_many(harness, arena, four(off), four(mask), four(h), four(tail), add, col(lambda g: g.hints), end, lanes)
    n_clean = 0
    for c, g in enumerate(regs):
        for k in range(4):
            bb = int(b[c, k])
            assert g.h <= bb <= g.tail
            assert bool(clean[c, k]) == bc.ref_clean(g.t, g.mask, g.h, g.tail, bb), (c, k, bb)     # the three pairs around the b it returned
            if clean[c, k]:
                n_clean += 1
                assert exact_partition(g.t, g.mask, g.h, g.tail, bb, add[c, k], g.end), (c, k, bb)
                if bb < g.tail:
                    assert t[c, k] == bits(g.t[bb & g.mask]) and lat[c, k] == bits(g.lat[bb & g.mask]), (c, k, bb)
    # ---- the repair of the drop boundaries that are not clean (search 2, as in retire_env), each on its own region
    rot = np.flatnonzero(~clean[:, 2])
    assert len(rot) >= 500 and n_clean >= 2000
    p, ci, ct, cl = fix_drop(harness, arena, off[rot], mask[rot], h[rot], tail[rot], b[rot, 2], dl[rot], end[rot], lanes)
    after = arena.cpu().numpy()
    want = host.copy()
    for i, c in enumerate(rot):
        g = regs[c]
        fx = bc.ref_fix(g.t, g.lat, g.mask, g.h, g.tail, int(b[c, 2]), g.dl, g.end)
        assert int(p[i]) == fx[0] and int(ci[i]) == fx[1] and ct[i] == bits(fx[2]) and cl[i] == bits(fx[3]), (c, int(b[c, 2]), int(p[i]), int(ci[i]), fx[:4])
        nt, nl = bc.ring_after(g, fx)
        want[g.off:g.off + g.size, 0], want[g.off:g.off + g.size, 1] = nt, nl
        assert exact_partition(nt, g.mask, g.h, g.tail, fx[0], g.dl, g.end), c      # over the WHOLE ring: [h, p) pass, [p, tail) fail
    assert np.array_equal(after.view(np.int64), want.view(np.int64))                # the windows partitioned bit for bit, nothing else touched
    # ---- the hop-1 candidate: after a repair from search_boundary(p, tail, 0, end); without one, where search 3 is not clean,
    # from its b (or p if that is above it)
    rotated = ~clean[:, 2]
    pd = b[:, 2].copy()
    pd[rot] = p
    cd = np.maximum(b[:, 3], pd)
    cd[rot] = search_boundary(harness, arena, off[rot], mask[rot], pd[rot], tail[rot], 0 * dl[rot], end[rot], lanes)
    need = np.flatnonzero((rotated | ~clean[:, 3]) & (tail != pd))
    assert len(need) >= 500 and (~rotated[need]).sum() >= 50
    ht, hl = hop1(harness, arena, off[need], mask[need], pd[need], tail[need], cd[need], end[need], lanes)
    for i, c in enumerate(need):
        g = regs[c]
        want_t, want_l = bc.scan_hop1(want[g.off:g.off + g.size, 0], want[g.off:g.off + g.size, 1], g.mask, int(pd[c]), g.tail, g.end)
        assert ht[i] == bits(want_t) and hl[i] == bits(want_l), (c, int(pd[c]), int(cd[c]), want_t, want_l)
    assert np.array_equal(arena.cpu().numpy().view(np.int64), want.view(np.int64))  # (neither of the two writes)


# ---------------------------------------------------------------------------------------------- the repairs, called directly
@pytest.fixture(scope="module")
def repaired(harness):
    """lanes -> what the two repairs returned on the repair table (hop 1 first: it only reads) and the arena after the fix"""
    cache = {}

    def get(lanes):
        if lanes not in cache:
            regs = bc.repair_table()
            arena = torch.as_tensor(region_arena(regs), device=DEV)
            col = lambda f: np.array([f(g) for g in regs])
            off, mask, h, tail, b = col(lambda g: g.off), col(lambda g: g.mask), col(lambda g: g.h), col(lambda g: g.tail), col(lambda g: g.b)
            h1 = hop1(harness, arena, off, mask, h, tail, b, col(lambda g: g.end1), lanes)
            fx = fix_drop(harness, arena, off, mask, h, tail, b, col(lambda g: g.dl), col(lambda g: g.end), lanes)
            cache[lanes] = (h1, fx, arena.cpu().numpy())
        return cache[lanes]
    return get


@pytest.mark.parametrize("lanes", [8, 16])
def test_repairs_equal_the_reference(repaired, lanes):
    """near windows of every size 1 .. 2 G + 4 (the ballot path, the lead lane's walk beyond G records), at h, at tail, wrapping: p, the
    hop-2 candidate (index, time, latency), the hop-1 candidate, and the whole region afterwards, bit for bit"""
    (ht, hl), (p, ci, ct, cl), after = repaired(lanes)
    regs, refs = bc.repair_table(), bc.repair_reference()
    want = np.empty_like(after)
    for i, (g, (fx, h1)) in enumerate(zip(regs, refs)):
        assert int(p[i]) == fx[0] and int(ci[i]) == fx[1] and ct[i] == bits(fx[2]) and cl[i] == bits(fx[3]), \
            (i, g.kind, g.cls, g.touch, g.w, g.b - g.ga, int(p[i]) - g.c0, int(ci[i]), fx[0] - g.c0, fx[1:6])
        assert ht[i] == bits(h1[0]) and hl[i] == bits(h1[1]), (i, g.kind, g.cls, g.touch, g.w, g.b - g.ga, h1)
        want[g.off:g.off + g.size, 0], want[g.off:g.off + g.size, 1] = bc.ring_after(g, fx)
    bad = np.flatnonzero((after.view(np.int64) != want.view(np.int64)).any(axis=1))
    assert bad.size == 0, "records that differ after the repair, first at arena record %d" % bad[0]


@pytest.mark.parametrize("lanes", [8, 16])
def test_repairs_do_not_depend_on_b(repaired, lanes):
    """Called with every b from the group's first record to one past its last, the repair leaves the same ring and the same p -- and
    the same candidate wherever the reference's own does not depend on b (boundary_cases.hop2_depends_on_b) --: what "the
    answer can be off inside one near group" relies on."""
    _, (p, ci, ct, cl), after = repaired(lanes)
    first, checked = {}, 0
    for i, g in enumerate(bc.repair_table()):
        region = after[g.off:g.off + g.size].view(np.int64)
        if g.family not in first:
            first[g.family] = (i, region)
            continue
        j, region0 = first[g.family]
        assert p[i] == p[j] and np.array_equal(region, region0), (g.family, g.b)
        if not bc.hop2_depends_on_b(g):
            assert ci[i] == ci[j] and ct[i] == ct[j] and cl[i] == cl[j], (g.family, g.b)
            checked += 1
    assert checked >= 5000


# ---------------------------------------------------------------------------------------------- arguments
def test_the_entry_points_refuse_what_they_cannot_run(harness):
    """refused on the host, without a launch: the outputs keep their prefill"""
    z = torch.zeros(64, dtype=torch.float64, device=DEV)
    arena = torch.zeros((16, 2), dtype=torch.float64, device=DEV)
    out = out_u32(64)
    zp, op = z.data_ptr(), out.data_ptr()
    entries = ((harness.pcc_test_search_many, 7, 4), (harness.pcc_test_search_boundary, 6, 1), (harness.pcc_test_fix_drop_boundary, 7, 4),
               (harness.pcc_test_drop_hop1_candidate, 6, 2))
    for fn, n_in, n_out in entries:
        good = lambda a=arena.data_ptr(), recs=16, n=1, lanes=8, ins=None, outs=None: fn(a, recs, *(ins or [zp] * n_in), n, lanes, *(outs or [op] * n_out), None)
        assert good(lanes=4) == HIP_ERROR_INVALID_VALUE and good(lanes=32) == HIP_ERROR_INVALID_VALUE        # lanes: 8 or 16
        assert good(a=None) == HIP_ERROR_INVALID_VALUE and good(recs=0) == HIP_ERROR_INVALID_VALUE           # no arena
        assert good(recs=(1 << 28) + 1) == HIP_ERROR_INVALID_VALUE
        assert good(n=-1) == HIP_ERROR_INVALID_VALUE
        assert good(ins=[zp] * (n_in - 1) + [None]) == HIP_ERROR_INVALID_VALUE and good(outs=[None] + [op] * (n_out - 1)) == HIP_ERROR_INVALID_VALUE
        assert good(n=0) == 0                                                                             # nothing to do: no launch either
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all()
    # a case whose ring does not lie in the arena is skipped on the device: mask + 1 = 32 records in an arena of 16
    idx = out_u32(1, 8)
    (got,) = call(harness.pcc_test_search_boundary, arena, [u32([0]), u32([31]), u32([0]), u32([4]), f64([0.0]), f64([1.0])], 1, 8, [idx])
    assert (got == -1).all()
