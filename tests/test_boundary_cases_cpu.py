"""The reference side of tests/test_retire_search.py, proved on the CPU from the case tables of tests/models/boundary_cases.py alone:
no device code is involved in anything this file asserts.

  1. coverage BY CONSTRUCTION: a few-line restatement of search_many's predicted window sorts every search of the table into hit /
     miss above / miss below by distance / no narrowing needed, and every class, every combination of the four searches of a
     group missing, every wrap of the masked index and every class of the repairs (window sizes around G, windows at h and at
     tail, b at every place, none / all / some of the window retiring, candidate ties) has at least FLOOR cases.  The floor is a
     cap on how thin the table may be, not a measurement: a table that does not meet it is changed until it does.
  2. the rings keep what the device code presumes: gaps far above the near tolerance, tie groups far below it.
  3. the reference checks itself: two codings of the partition agree on every case, and the result of a repair does not depend
     on which b of the near group it was called with (where it cannot: boundary_cases.hop2_depends_on_b)."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import boundary_cases as bc   # noqa: E402

FLOOR = 50
GS = (8, 16)


# ------------------------------------------------------------------------------------------------ 1. the searches
def predicted_window(lo0, hi0, hint):
    h = min(max(hint, lo0), hi0)
    lo = h - 5 if h - lo0 >= 5 else lo0
    hi = lo + 12 if hi0 - lo > 12 else hi0
    return lo, hi


def search_class(ring, lo0, hi0, add, hint, end, b):
    """'hit', 'short-above' / 'short-below' (the range left after the miss is <= 12: the final window, no narrowing), or
    ('above' | 'below', bin) with bin = the first of 12, 48, 192, 768, inf that the distance from the window's edge fits under"""
    passes = lambda k: ring.t[k & ring.mask] + add < end
    lo, hi = predicted_window(lo0, hi0, hint)
    lo_ok = lo == lo0 or passes(lo - 1)
    hi_ok = hi == hi0 or not passes(hi)
    if lo_ok and hi_ok:
        return "hit"
    (side, lo_m, hi_m) = ("below", lo0, lo - 1) if not lo_ok else ("above", hi + 1, hi0)
    assert lo_m <= b <= hi_m
    if hi_m - lo_m <= 12:
        return "short-" + side
    d = hi_m - b if side == "below" else b - lo_m
    return side, next(x for x in (12, 48, 192, 768, np.inf) if d <= x)


def wraps(ring, first, n):
    """the masked index wraps inside [first, first + n)"""
    return n > 1 and (first & ring.mask) > ((first + n - 1) & ring.mask)


def classes_of_searches():
    tab, rings = bc.search_table(), bc.accepted_rings()
    b = bc.search_reference()[0]
    out = []
    for c in range(len(tab["end"])):
        out.append([search_class(rings[tab["ring"][c, k]], int(tab["lo0"][c, k]), int(tab["hi0"][c, k]), tab["add"][c, k],
                                 int(tab["hint"][c, k]), tab["end"][c], int(b[c, k])) for k in range(4)])
    return out


def test_every_search_class_has_its_cases():
    cls = classes_of_searches()
    count = collections.Counter(x for row in cls for x in row)
    want = ["hit", "short-above", "short-below"] + [(s, d) for s in ("above", "below") for d in (12, 48, 192, 768, np.inf)]
    print(sorted(count.items(), key=str))
    for w in want:
        assert count[w] >= FLOOR, (w, count[w])
    # 0, 1, 2, 3 and 4 searches of a group miss, in every combination (a group that returns next to one that descends: the order
    # of the cases in a launch is the test's, tests/test_retire_search.py)
    combos = collections.Counter(tuple(x != "hit" for x in row) for row in cls)
    print(sorted(combos.items()))
    assert len(combos) == 16 and min(combos.values()) >= FLOOR, combos
    # ... and, among the groups that descend, every combination of above / below in two searches side by side
    sides = collections.Counter((row[k][0], row[k + 1][0]) for row in cls for k in range(3) if isinstance(row[k], tuple) and isinstance(row[k + 1], tuple))
    assert len(sides) == 4 and min(sides.values()) >= FLOOR, sides


def test_the_search_table_has_the_ranges_boundaries_and_hints_it_names():
    tab, rings = bc.search_table(), bc.accepted_rings()
    b, clean, _, _ = bc.search_reference()
    assert clean.all()                                  # accepted-like: nothing is near anything
    n = tab["hi0"] - tab["lo0"]
    for r in bc.RANGES:
        assert (n == r).sum() >= FLOOR, r
    beta = b - tab["lo0"]
    big = n >= 11
    for name, sel in (("at lo0", beta == 0), ("at hi0", beta == n), ("lo0 + 1", beta == 1), ("hi0 - 1", beta == n - 1), ("middle", (beta > 1) & (beta < n - 1))):
        assert (sel & big).sum() >= FLOOR, name
    # `end` equal to t + add of the boundary record: `<=` for `<` would move the boundary
    eq = 0
    for c in range(len(tab["end"])):
        for k in range(4):
            r = rings[tab["ring"][c, k]]
            eq += b[c, k] < tab["hi0"][c, k] and r.t[b[c, k] & r.mask] + tab["add"][c, k] == tab["end"][c]
    assert eq >= 10 * FLOOR, eq
    off = tab["hint"] - b
    for o in bc.HINT_OFFSETS:
        for s in (1, -1):
            assert (off == s * o).sum() >= (FLOOR if o < 3000 else 10), (s * o, (off == s * o).sum())
    assert (tab["hint"] < tab["lo0"]).sum() >= FLOOR and (tab["hint"] > tab["hi0"]).sum() >= FLOOR
    assert (tab["hint"] == 0).sum() >= FLOOR and (tab["hint"] == bc.NONE).sum() >= FLOOR
    assert set(np.unique(tab["add"][:, 0])) == set(bc.DLS) and not tab["add"][:, 1::2].any() and (tab["add"][:, 2] == tab["dl"]).all()
    assert set(rings[i].size for i in np.unique(tab["ring"])) == set(bc.RING_SIZES)
    assert tab["hi0"].max() < 2 ** 31                   # no cursor near 2**32


def test_the_masked_index_wraps_inside_the_windows():
    tab, rings = bc.search_table(), bc.accepted_rings()
    b = bc.search_reference()[0]
    first = final = probes = 0
    for c in range(len(tab["end"])):
        for k in range(4):
            r, lo0, hi0 = rings[tab["ring"][c, k]], int(tab["lo0"][c, k]), int(tab["hi0"][c, k])
            lo, _ = predicted_window(lo0, hi0, int(tab["hint"][c, k]))
            base = lo - 2 if lo - lo0 >= 2 else lo0
            first += wraps(r, base, min(16, hi0 - base))
            bb = int(b[c, k])
            base = max(bb - 14, lo0)                    # (the final window starts at most 14 records under the boundary)
            final += wraps(r, max(bb - 2, lo0), min(4, hi0 - max(bb - 2, lo0)))
            probes += wraps(r, lo0, hi0 - lo0) and hi0 - lo0 > 16
    assert first >= FLOOR and final >= FLOOR and probes >= FLOOR, (first, final, probes)


# ------------------------------------------------------------------------------------------------ 1. the repairs
def repair_classes(G):
    """Counter of the classes of the cases of the repair table at G lanes, from the reference's near window alone"""
    count = collections.Counter()
    for g, (fx, _) in zip(bc.repair_table(), bc.repair_reference()):
        g0, g1 = fx[4], fx[5]
        n = g1 - g0
        count["size", n] += 1
        count["size", "<G" if n < G else "=G" if n == G else "G+1" if n == G + 1 else ">G+1"] += 1
        count["touch", g0 == g.h, g1 == g.tail] += 1
        count["b", "first" if g.b == g0 else "end" if g.b == g1 else "inside"] += 1
        wt = [g.t[k & g.mask] for k in range(g0, g1)]
        ok = [x + g.dl < g.end for x in wt]
        count["retire", "none" if not any(ok) else "all" if all(ok) else "mixed"] += 1
        count["retire", "none" if not any(ok) else "all" if all(ok) else "mixed", "serial" if n > G else "group"] += 1
        ok1 = [x < g.end1 for x in wt]
        count["hop1", "none" if not any(ok1) else "all" if all(ok1) else "mixed", "serial" if n > G else "group"] += 1
        count["wrap"] += wraps(g, g0, n)
        count["h inside a tie group"] += g0 == g.h and g.h > g.c0 and bc.near_time(g.t[(g.h - 1) & g.mask], g.t[g.h & g.mask])
        count["tail inside a tie group"] += g1 == g.tail and g.tail < g.c0 + len(g.T) and bc.near_time(g.t[(g.tail - 1) & g.mask], g.t[g.tail & g.mask])
        # the hop-2 key (t + dl, lat + dl) orders the window differently from the hop-1 key (t, lat): t + dl rounds two times that
        # differ into one, and the latencies order that pair the other way
        wl = [g.lat[k & g.mask] for k in range(g0, g1)]
        k1 = sorted(range(n), key=lambda i: (wt[i], wl[i], i))
        k2 = sorted(range(n), key=lambda i: (wt[i] + g.dl, wl[i] + g.dl, i))
        count["orders differ"] += k1 != k2
        p = fx[0]
        new_t, new_l = fx[6], fx[7]
        count["hop2 tie", bc.tie_class([(new_t[j] + g.dl, new_l[j] + g.dl) for j in range(p - g0, n) if new_t[j] < g.end]), "serial" if n > G else "group"] += 1
        count["hop1 tie", bc.tie_class([(wt[j], wl[j]) for j in range(n) if not (wt[j] < g.end1)]), "serial" if n > G else "group"] += 1
    return count


def test_every_repair_class_has_its_cases():
    for G in GS:
        count = repair_classes(G)
        print(G, sorted(count.items(), key=str))
        for n in range(1, 2 * G + 5):
            assert count["size", n] >= FLOOR, (G, n, count["size", n])
        for s in ("<G", "=G", "G+1", ">G+1"):
            assert count["size", s] >= FLOOR, (G, s)
        for a in (False, True):
            for b in (False, True):
                assert count["touch", a, b] >= FLOOR, (G, a, b)
        for b in ("first", "inside", "end"):
            assert count["b", b] >= FLOOR
        for r in ("none", "all", "mixed"):
            for path in ("group", "serial"):
                assert count["retire", r, path] >= FLOOR and count["hop1", r, path] >= FLOOR, (G, r, path)
        assert count["wrap"] >= FLOOR and count["h inside a tie group"] >= FLOOR and count["tail inside a tie group"] >= FLOOR
        assert count["orders differ"] >= 100
        for hop in ("hop2 tie", "hop1 tie"):
            for how in ("time", "lat", "order", None):
                for path in ("group", "serial"):
                    assert count[hop, how, path] >= FLOOR, (G, hop, how, path, count[hop, how, path])


def test_the_flow_table_cuts_tie_groups():
    """the whole-flow cases: how many drop boundaries are not clean by the reference's own scan (those go through the repair), how
    many regions wrap inside [h, tail), how many ranges are empty"""
    dirty = wrap = 0
    for g in bc.flow_table():
        b, clean, _, _ = bc.ref_search(g.t, g.lat, g.mask, g.h, g.tail, g.dl, g.end)
        dirty += not clean
        wrap += wraps(g, g.h, g.tail - g.h)
    assert dirty >= 10 * FLOOR and len(bc.flow_table()) - dirty >= 10 * FLOOR and wrap >= 10 * FLOOR, (dirty, wrap)


# ------------------------------------------------------------------------------------------------ 2. ring invariants
def assert_dropped_invariants(g):
    """along the ring: neighbours are either within the few-ulp spread of a tie group or further apart than 64 * kNearTol * t --
    nothing sits where near_time's two argument orders, or rounding, could disagree"""
    T = g.T
    d = np.abs(np.diff(T))
    tie = d <= 6 * np.spacing(np.maximum(T[1:], T[:-1]))
    gap = d >= np.maximum(64 * bc.NEAR_TOL * np.maximum(1.0, np.abs(T[1:])), 1e-3 - 1e-9)
    assert (tie | gap).all() and (np.diff(T)[~tie] > 0).all()
    assert all(bc.near_time(T[i], T[i + 1]) and bc.near_time(T[i + 1], T[i]) for i in np.flatnonzero(tie))
    assert not any(bc.near_time(T[i], T[i + 1]) or bc.near_time(T[i + 1], T[i]) for i in np.flatnonzero(~tie))
    run = np.diff(np.flatnonzero(np.concatenate(([True], ~tie, [True]))))
    assert run.max() <= 46                              # a group of 40, or a designated one of 36 going on past both cursors
    assert T.max() <= 1e4 and T.min() > 0


def test_ring_invariants():
    for r in bc.accepted_rings():
        d = np.diff(r.T)
        assert (d >= 1e-3).all() and (d >= 64 * bc.NEAR_TOL * r.T[1:]).all() and r.T[-1] <= 1e4 and r.T[0] > 0
        assert (r.c0 & r.mask) != 0 and r.c0 < r.wrap < r.c0 + r.size
    lat = np.concatenate([r.LAT for r in bc.accepted_rings()])
    assert len(np.unique(lat)) == len(lat)
    seen = set()
    for g in bc.repair_table():
        if g.family not in seen:                        # (the cases of a family share their ring's contents)
            seen.add(g.family)
            assert_dropped_invariants(g)
        assert g.c0 <= g.h <= g.b <= g.tail <= g.c0 + len(g.T) <= g.c0 + g.size and g.size in (64, 128, 256)
    for g in bc.flow_table():
        assert_dropped_invariants(g)
        assert g.c0 <= g.h <= g.tail <= g.c0 + len(g.T) <= g.c0 + g.size and g.size in (64, 128, 256)
        assert len(np.unique(g.LAT)) == len(g.LAT)
    sizes = collections.Counter()
    for g in bc.flow_table():
        tie = np.abs(np.diff(g.T)) < 1e-6
        for n in np.diff(np.flatnonzero(np.concatenate(([True], ~tie, [True])))):
            sizes[int(n)] += 1
    assert set(sizes) == set(range(1, 41))


# ------------------------------------------------------------------------------------------------ 3. the reference checks itself
def test_two_codings_of_the_partition_agree():
    for g, (fx, _) in zip(bc.repair_table(), bc.repair_reference()):
        p, wt, wl = bc.partition_by_moves(g.t, g.lat, g.mask, fx[4], fx[5], g.dl, g.end)
        assert p == fx[0] and np.array_equal(wt.view(np.int64), fx[6].view(np.int64)) and np.array_equal(wl.view(np.int64), fx[7].view(np.int64)), (g.family, g.b)
    for g in bc.flow_table():
        for b in (g.h, (g.h + g.tail) // 2, g.tail):
            fx = bc.ref_fix(g.t, g.lat, g.mask, g.h, g.tail, b, g.dl, g.end)
            p, wt, wl = bc.partition_by_moves(g.t, g.lat, g.mask, fx[4], fx[5], g.dl, g.end)
            assert p == fx[0] and np.array_equal(wt.view(np.int64), fx[6].view(np.int64)) and np.array_equal(wl.view(np.int64), fx[7].view(np.int64))


def test_the_reference_does_not_depend_on_b():
    """Within a family (the same ring, cursors, dl and end; b = every cursor from the designated group's first record to one past its
    last) the ring afterwards and p are the same whatever b; so are the candidates wherever the cut goes through the group or
    under it.  tests/test_retire_search.py holds the device to the same."""
    fams = collections.defaultdict(list)
    for g, ref in zip(bc.repair_table(), bc.repair_reference()):
        fams[g.family].append((g, ref))
    held = 0
    for fam in fams.values():
        g0, (fx0, _) = fam[0]
        t0, l0 = bc.ring_after(g0, fx0)
        assert len(fam) == g0.gb - g0.ga + 1 and [g.b for g, _ in fam] == list(range(g0.ga, g0.gb + 1))
        for g, (fx, _) in fam[1:]:
            t, lat = bc.ring_after(g, fx)
            assert fx[0] == fx0[0] and np.array_equal(t.view(np.int64), t0.view(np.int64)) and np.array_equal(lat.view(np.int64), l0.view(np.int64)), g.family
            if not bc.hop2_depends_on_b(g):
                assert fx[1:4] == fx0[1:4], (g.family, g.b)
                held += 1
    assert held >= 100 * FLOOR
