"""The case tables and the plain reference of tests/test_boundary_cases_cpu.py (which proves their coverage on the CPU, from the inputs
alone) and of tests/test_retire_search.py (which runs them through tests/kernels/retire_search_harness.hip): the boundary searches
search_many<4, G> / search_boundary<G> and the near-group repairs fix_drop_boundary_g<G> / drop_hop1_candidate_g<G> of
pcc-rl_amd/csrc/pcc_retire_env.h.  numpy only.

A RING is `size` (a power of two, 16 .. 8192) records (t1, lat); record of cursor k sits at position k & (size - 1), and a ring
holds the cursors [c0, c0 + size) with c0 chosen so that the masked index wraps inside it.  All rings of a table lie in one ARENA
(`off` = the ring's first record in it).  Cursors just below 2**32 are not in the tables: the code compares cursors with `<` and
the product resets them to 0 long before.

  accepted-like   strictly increasing t1 over about [1, 5000] whatever the size (so one `end` cuts every ring somewhere), gaps
                  >= 1e-3; shared, read-only.
  dropped-like    tie groups of 1 .. 40 records, the groups spaced like accepted records; inside a group the times are ONE value
                  perturbed by -3 .. +3 ulps in shuffled order.  A repair rewrites its ring, so every
                  case has a region of 64 .. 256 records of its own.
  lat             distinct for every record of an arena (a wrong record shows), except where a case plants a tie on purpose.

THE REFERENCE is linear scans in float64 with the expressions of the device code (`t + add < end`; near_time(a, b) =
|a - b| <= 1e-12 * max(1, |b|)):
  search          b = the first index of [lo0, hi0) that fails `t + add < end`, hi0 if none fails; (t, lat) = ring[b] when b < hi0;
                  clean iff no k of {b - 2, b - 1, b} has k >= lo0, k + 1 < hi0 and near_time(t[k], t[k + 1]).  (Re-derived from
                  window(): its 16 records start at base = max(lo - 2, lo0) with b in [lo, lo + 12], so the three pairs it
                  looks at are inside it exactly when k >= lo0, and pair b's second record is at most record 15.)
  near window     [g0, g1) around b, h <= g0 <= b <= g1 <= tail: b - 1 and b themselves (where they exist) and everything chained
                  to them by near pairs; downwards a pair is tested as near_time(earlier, later), upwards as near_time(later, earlier),
                  as the device does (the two differ only within rounding of the tolerance itself, 1e-12 relative: the rings'
                  invariants keep every pair three orders of magnitude away from it on either side).
  fix             the window stably partitioned on `t + dl < end`, p = g0 + the number that pass; the hop-2 candidate = the minimum
                  of (t + dl, lat + dl, position after the partition) over the window's unretired records with `t < end`.
  hop 1           the minimum of (t, lat) over the window's records with `!(t < end)`.
A candidate that does not exist is (0xFFFFFFFF, inf, 0.0)."""
import functools

import numpy as np

NEAR_TOL = 1e-12
NONE = 0xFFFFFFFF
RANGES = (0, 1, 2, 11, 12, 13, 16, 17, 100, 1000, 5000)
RANGE_WEIGHTS = (1, 1, 1, 1, 1, 1, 1, 1, 3, 6, 6)
HINT_OFFSETS = (0, 1, 4, 5, 6, 7, 8, 12, 13, 47, 48, 49, 191, 192, 193, 767, 768, 769, 3000)
RING_SIZES = tuple(1 << k for k in range(4, 14))   # 16 .. 8192
RING_VARIANTS = 3
DLS = (0.03, 0.1, 0.2999)
N_SEARCH_CASES = 3000
MAX_WINDOW = 2 * 16 + 4                            # the repairs: near windows of every size 1 .. 2 G + 4
N_FLOW_CASES = 2500
SEED = 31


def near_time(a, b):
    return abs(a - b) <= NEAR_TOL * max(1.0, abs(b))


# ------------------------------------------------------------------------------------------------------------------ reference
def ref_search(t, lat, mask, lo0, hi0, add, end):
    """(b, clean, t[b], lat[b]) by linear scan; t, lat: the ring by position.  (t[b], lat[b]) is (nan, nan) when b == hi0."""
    b = hi0
    for k in range(lo0, hi0):
        if not (t[k & mask] + add < end):
            b = k
            break
    return (b, ref_clean(t, mask, lo0, hi0, b)) + ((float(t[b & mask]), float(lat[b & mask])) if b < hi0 else (np.nan, np.nan))


def ref_clean(t, mask, lo0, hi0, b):
    for k in (b - 2, b - 1, b):
        if k >= lo0 and k + 1 < hi0 and near_time(t[k & mask], t[(k + 1) & mask]):
            return False
    return True


def ref_near_window(t, mask, h, tail, b):
    g0 = g1 = b
    if b > h:
        g0 = b - 1
        while g0 > h and near_time(t[(g0 - 1) & mask], t[g0 & mask]):     # (earlier, later)
            g0 -= 1
    if b < tail:
        g1 = b + 1
        while g1 < tail and near_time(t[g1 & mask], t[(g1 - 1) & mask]):  # (later, earlier)
            g1 += 1
    return g0, g1


def ref_fix(t, lat, mask, h, tail, b, dl, end):
    """-> (p, cand_idx, cand_t, cand_lat, g0, g1, wt, wl): wt, wl = the window's records after the stable partition (a filter: the
    passing records in their order, then the others in theirs)."""
    g0, g1 = ref_near_window(t, mask, h, tail, b)
    rec = [(float(t[k & mask]), float(lat[k & mask])) for k in range(g0, g1)]
    front = [r for r in rec if r[0] + dl < end]
    back = [r for r in rec if not (r[0] + dl < end)]
    p = g0 + len(front)
    best = None
    for j, r in enumerate(back):
        if r[0] < end:
            key = (r[0] + dl, r[1] + dl, p + j)
            if best is None or key < best:
                best = key
    new = front + back
    cand = (best[2], best[0], best[1]) if best is not None else (NONE, np.inf, 0.0)
    return (p,) + cand + (g0, g1, np.array([r[0] for r in new]), np.array([r[1] for r in new]))


def partition_by_moves(t, lat, mask, g0, g1, dl, end):
    """The second coding of the partition, as fix_drop_window does it: every passing record is moved in front of the first one
    that does not pass, one by one, the records in between shifted up.  -> (p, wt, wl)"""
    wt = [float(t[k & mask]) for k in range(g0, g1)]
    wl = [float(lat[k & mask]) for k in range(g0, g1)]
    p = 0
    for k in range(len(wt)):
        if wt[k] + dl < end:
            if k != p:
                rt, rl = wt[k], wl[k]
                for m in range(k, p, -1):
                    wt[m], wl[m] = wt[m - 1], wl[m - 1]
                wt[p], wl[p] = rt, rl
            p += 1
    return g0 + p, np.array(wt), np.array(wl)


def ref_hop1(t, lat, mask, h, tail, c, end):
    g0, g1 = ref_near_window(t, mask, h, tail, c)
    return scan_hop1(t, lat, mask, g0, g1, end)


def scan_hop1(t, lat, mask, lo, hi, end):
    """the minimum of (t, lat) over the records of [lo, hi) with !(t < end); (inf, 0.0) if there is none"""
    best = None
    for k in range(lo, hi):
        r = (float(t[k & mask]), float(lat[k & mask]))
        if not (r[0] < end) and (best is None or r < best):
            best = r
    return best if best is not None else (np.inf, 0.0)


# ------------------------------------------------------------------------------------------------------------------ accepted-like rings
class Ring:
    """t, lat by POSITION; T by cursor order (T[i] = the time of cursor c0 + i)"""

    def __init__(self, size, c0, off, T, LAT):
        self.size, self.mask, self.c0, self.off, self.T, self.LAT = size, size - 1, c0, off, T, LAT
        pos = (c0 + np.arange(size)) & (size - 1)
        self.t = np.empty(size)
        self.lat = np.empty(size)
        self.t[pos] = T
        self.lat[pos] = LAT
        self.wrap = c0 + (size - (c0 & (size - 1)))   # the first cursor that sits at position 0 again (c0 is never a multiple of size)


@functools.lru_cache(maxsize=None)
def accepted_rings():
    rs = np.random.RandomState(SEED)
    out, off = [], 0
    for size in RING_SIZES:
        for v in range(RING_VARIANTS):
            gaps = 1e-3 + rs.rand(size) * 2.0 * (4990.0 / size - 1e-3)
            T = 1.0 + np.cumsum(gaps)
            LAT = 0.01 + 1e-6 * (off + 1 + rs.permutation(size))
            c0 = size * (v + 1) + int(rs.randint(1, size))
            out.append(Ring(size, c0, off, T, LAT))
            off += size
    return out


def arena_of(rings):
    """(records, 2) float64: the rings one after the other"""
    a = np.empty((sum(r.size for r in rings), 2))
    for r in rings:
        a[r.off:r.off + r.size, 0] = r.t
        a[r.off:r.off + r.size, 1] = r.lat
    return a


def _passing(ring, add, end):
    """how many records of the ring, from cursor c0 on, pass `T + add < end` (the ring is monotone: they are a prefix)"""
    ok = ring.T + add < end
    return int(ring.size if ok.all() else np.argmin(ok))


def _beta(rs, n):
    kind = rs.randint(5)
    return (0, n, min(1, n), max(n - 1, 0), int(rs.randint(0, n + 1)))[kind]


def _hint(rs, b, lo0, hi0):
    u = rs.rand()
    if u < 0.72:
        o = HINT_OFFSETS[rs.randint(len(HINT_OFFSETS))] * (1 if rs.rand() < 0.5 else -1)
        return max(b + o, 0)
    if u < 0.82:
        return max(lo0 - int(rs.randint(1, 60)), 0)
    if u < 0.92:
        return hi0 + int(rs.randint(1, 60))
    return 0 if u < 0.96 else NONE


@functools.lru_cache(maxsize=None)
def search_table():
    """The cases of search_many on the accepted-like rings: dict of arrays -- ring (index into accepted_rings()), lo0, hi0, add, hint
    of shape (cases, 4); end, dl of shape (cases,).  The four searches of a case take their range size, the place of the boundary
    in it and their hint independently; the adds are (dl, 0, dl, 0) as the product passes them; `end` is, for two cases of three,
    exactly t + add of a record of one of the four (so `<` against `<=` shows), otherwise half-way between two records."""
    rs = np.random.RandomState(SEED + 1)
    rings = accepted_rings()
    pw = np.array(RANGE_WEIGHTS, dtype=float) / sum(RANGE_WEIGHTS)
    K = N_SEARCH_CASES
    tab = {"ring": np.zeros((K, 4), np.int64), "lo0": np.zeros((K, 4), np.int64), "hi0": np.zeros((K, 4), np.int64),
           "add": np.zeros((K, 4)), "hint": np.zeros((K, 4), np.int64), "end": np.zeros(K), "dl": np.zeros(K)}
    for c in range(K):
        dl = DLS[rs.randint(len(DLS))]
        adds = (dl, 0.0, dl, 0.0)
        # the anchor search fixes `end`: its boundary is record j of its ring
        q = int(rs.randint(4))
        n = int(rs.choice(RANGES, p=pw))
        beta = _beta(rs, n)
        ring_q = int(rs.choice([i for i, r in enumerate(rings) if r.size >= n]))
        r = rings[ring_q]
        jlo, jhi = beta, r.size - (n - beta)                 # record j with beta records of the range below it, n - beta from it on
        j = int(rs.randint(jlo, jhi + 1))
        if rs.rand() < 0.4:                                  # the masked index wraps in the windows around the boundary
            j = int(np.clip(r.wrap - r.c0 + rs.randint(-14, 4), jlo, jhi))
        if j == r.size:
            end = r.T[-1] + adds[q] + 5e-4
        elif rs.rand() < 0.67 or j == 0:
            end = r.T[j] + adds[q]
        else:
            end = 0.5 * ((r.T[j - 1] + adds[q]) + (r.T[j] + adds[q]))
        tab["end"][c], tab["dl"][c] = end, dl
        for k in range(4):
            if k == q:
                ri, nk, bk, B = ring_q, n, beta, _passing(r, adds[k], end)
            else:
                for _ in range(40):
                    nk = int(rs.choice(RANGES, p=pw))
                    bk = _beta(rs, nk)
                    ri = int(rs.choice([i for i, x in enumerate(rings) if x.size >= nk]))
                    B = _passing(rings[ri], adds[k], end)
                    if bk <= B and nk - bk <= rings[ri].size - B:
                        break
                else:
                    nk, bk = 0, 0
            rk = rings[ri]
            lo0 = rk.c0 + B - bk
            tab["ring"][c, k], tab["lo0"][c, k], tab["hi0"][c, k], tab["add"][c, k] = ri, lo0, lo0 + nk, adds[k]
            tab["hint"][c, k] = _hint(rs, rk.c0 + B, lo0, lo0 + nk)
    return tab


@functools.lru_cache(maxsize=None)
def search_reference():
    """(b, clean, t, lat), each of shape (cases, 4), by linear scan"""
    tab, rings = search_table(), accepted_rings()
    K = len(tab["end"])
    b, clean, t, lat = np.zeros((K, 4), np.int64), np.zeros((K, 4), bool), np.zeros((K, 4)), np.zeros((K, 4))
    for c in range(K):
        for k in range(4):
            r = rings[tab["ring"][c, k]]
            b[c, k], clean[c, k], t[c, k], lat[c, k] = ref_search(r.t, r.lat, r.mask, int(tab["lo0"][c, k]), int(tab["hi0"][c, k]),
                                                                   tab["add"][c, k], tab["end"][c])
    return b, clean, t, lat


# ------------------------------------------------------------------------------------------------------------------ dropped-like regions
def _tie_group(rs, v, n):
    """n times: v perturbed by -3 .. +3 ulps, in shuffled order"""
    return v + rs.randint(-3, 4, size=n) * np.spacing(v)


def _groups(rs, sizes, t0, gap):
    """(T, gid) in cursor order: tie groups of the given sizes, the first at about t0, spaced by 1e-3 + U(0, gap)"""
    T, gid, v = [], [], t0
    for i, n in enumerate(sizes):
        T.append(_tie_group(rs, v, n))
        gid += [i] * n
        v = v + 1e-3 + rs.rand() * gap
    return np.concatenate(T), np.array(gid)


class Region:
    """one case's private ring: fields as Ring's, plus the case's h, tail, b, dl, end, end1 (the `end` of its hop-1 call), its family
    (cases of a family differ in b alone) and the designated group's cursors [ga, gb)"""


def _region(size, c0, T, LAT):
    g = Region()
    g.size, g.mask, g.c0, g.T, g.LAT = size, size - 1, c0, T, LAT
    pos = (c0 + np.arange(len(T))) & (size - 1)
    g.t = np.full(size, 9e9)       # (positions outside the cursors in use: later than everything, never near anything)
    g.lat = np.full(size, 7.0)
    g.t[pos] = T
    g.lat[pos] = LAT
    return g


def _size_for(n):
    return 64 if n <= 64 else 128 if n <= 128 else 256


def _cut(rs, s, cls, below, above):
    """an `end` for the values s of the designated group: none / all / a mixed subset of them pass `s < end`; below / above = the
    neighbouring groups' nearest values"""
    u = np.unique(s)
    if cls == "mixed" and len(u) >= 2:
        return float(u[rs.randint(1, len(u))])                        # == one of the values: that one fails, the smaller ones pass
    if cls == "all":
        return float(np.nextafter(u[-1], np.inf)) if rs.rand() < 0.5 else float(0.5 * (u[-1] + above))
    return float(u[0]) if rs.rand() < 0.5 else float(0.5 * (below + u[0]))


@functools.lru_cache(maxsize=None)
def repair_table():
    """The cases of the repairs called directly: a designated tie group of every size 1 .. 2 * 16 + 4 (its neighbours are groups of
    1 .. 12), h and tail at its edges or away from them -- or INSIDE a tie group, which then goes on beyond the cursor --, `end`
    cutting none, all or a mixed subset of it, times ordinary or small against dl (where t + dl collapses times that differ), dl == 0, planted ties of (t) and of (t, lat), and, per such FAMILY, one case for every b from the group's first
    record to one past its last.  -> list of Region."""
    rs = np.random.RandomState(SEED + 2)
    out, fam, serial = [], 0, 0
    for w in range(1, MAX_WINDOW + 1):
        for touch in ("neither", "h", "tail", "both"):
            for cls in ("none", "all", "mixed"):
                for kind in ("ordinary", "small", "nodelay", "ties"):
                    ti, ci = ("neither", "h", "tail", "both").index(touch), ("none", "all", "mixed").index(cls)
                    if (w + ti + ci) % (2 if kind == "ordinary" else 3) != 0 and not (kind == "ties" and cls == "none"):
                        continue                                  # (half / a third of the combinations of a size per kind)
                    for rep in range(8 if w <= 2 else 4 if w <= 4 else 2 if w <= 8 else 1):   # (short groups have few b: more families of them)
                      a1, a2, n1, n2 = (int(x) for x in rs.randint(1, 13, size=4))
                      # the designated group goes on below h / beyond tail by xl / xr records: the cursor cuts a tie group
                      xl = int(rs.randint(1, 6)) if touch in ("h", "both") and rs.rand() < 0.5 else 0
                      xr = int(rs.randint(1, 6)) if touch in ("tail", "both") and rs.rand() < 0.5 else 0
                      sizes = [a1, a2, xl + w + xr, n1, n2]
                      t0 = 0.004 if kind == "small" else float(rs.uniform(1.0, 9000.0))
                      T, gid = _groups(rs, sizes, t0, 0.004 if kind == "small" else 0.5)
                      n = len(T)
                      LAT = 0.01 + 1e-6 * (serial + 1 + rs.permutation(n))
                      serial += n
                      ia = a1 + a2 + xl                             # [ia, ib): the w records of the designated group inside [h, tail)
                      ib = ia + w
                      if kind == "ties" and w >= 2:                 # several records share the group's smallest time, two of them maybe the latency too
                          m = np.flatnonzero(rs.rand(w) < 0.5)
                          if len(m) < 2:
                              m = rs.choice(w, 2, replace=False)
                          T[ia + m] = T[ia:ib].min()
                          if rs.rand() < 0.6:
                              LAT[ia + m[:2]] = LAT[ia:ib].min() - 1e-7
                      size = _size_for(n)
                      c0 = size * int(rs.randint(1, 4)) + int(rs.randint(1, size))
                      if rs.rand() < 0.6:                           # the masked index wraps inside the near window
                          c0 = size * int(rs.randint(1, 4)) + ((size - ia - int(rs.randint(0, w + 1))) % size or 1)
                      h = c0 + (ia if touch in ("h", "both") else int(rs.randint(0, a1 + 1)))
                      tail = c0 + (ib if touch in ("tail", "both") else ib + n1 + int(rs.randint(0, n2 + 1)))
                      dl = 0.0 if kind == "nodelay" else DLS[rs.randint(len(DLS))]
                      grp = T[ia:ib]
                      below, above = T[gid == 1].max(), T[gid == 3].min()
                      end = _cut(rs, grp + dl, cls, below + dl, above + dl)
                      end1 = _cut(rs, grp, cls, below, above)
                      for b in range(ia, ib + 1):
                          g = _region(size, c0, T, LAT)
                          g.h, g.tail, g.b, g.dl, g.end, g.end1, g.family, g.ga, g.gb = h, tail, c0 + b, dl, end, end1, fam, c0 + ia, c0 + ib
                          g.kind, g.cls, g.touch, g.w = kind, cls, touch, w
                          out.append(g)
                      fam += 1
    off = 0
    for g in out:
        g.off = off
        off += g.size
    return out


@functools.lru_cache(maxsize=None)
def flow_table():
    """The cases of the whole dropped-ring flow of retire_env (search_many; where the drop boundary is not clean,
    fix_drop_boundary_g, search_boundary and drop_hop1_candidate_g): regions full of random tie groups, [h, tail) anywhere, `end`
    cutting a random group on t + dl (two cases of three) or on t, four hints.  -> list of Region (b unused; hints = its four)."""
    rs = np.random.RandomState(SEED + 3)
    out, off, serial = [], 0, 0
    for c in range(N_FLOW_CASES):
        size = (64, 128, 256)[rs.randint(3)]
        sizes = []
        lone = (0.0, 0.5, 0.9)[rs.randint(3)]            # how many of the groups are single records: a clean boundary needs a few in a row
        while sum(sizes) < size - 40:
            sizes.append(1 if rs.rand() < lone else int(rs.randint(1, 41)) if rs.rand() < 0.3 else int(rs.randint(1, 7)))
        small = rs.rand() < 0.25
        T, gid = _groups(rs, sizes, 0.004 if small else float(rs.uniform(1.0, 9000.0)), 0.004 if small else 0.5)
        n = len(T)
        LAT = 0.01 + 1e-6 * (serial + 1 + rs.permutation(n))
        serial += n
        c0 = size * int(rs.randint(1, 4)) + int(rs.randint(1, size))
        g = _region(size, c0, T, LAT)
        a, b = sorted(int(x) for x in rs.randint(0, n + 1, size=2))
        if rs.rand() < 0.5:
            a, b = int(rs.randint(0, 4)), n - int(rs.randint(0, 4))
        g.h, g.tail = c0 + a, c0 + b
        g.dl = DLS[rs.randint(len(DLS))]
        d = int(rs.randint(len(sizes)))
        grp = T[gid == d]
        cls = ("none", "all", "mixed", "mixed")[rs.randint(4)]
        onsum = rs.rand() < 0.67
        g.end = _cut(rs, grp + (g.dl if onsum else 0.0), cls, grp.min() - 5e-4 + (g.dl if onsum else 0.0), grp.max() + 5e-4 + (g.dl if onsum else 0.0))
        # the boundaries by linear scan, for the hints only
        ok2, ok1 = T + g.dl < g.end, T < g.end
        b2 = a + int(np.argmin(ok2[a:b])) if b > a and not ok2[a:b].all() else b
        b1 = a + int(np.argmin(ok1[a:b])) if b > a and not ok1[a:b].all() else b
        g.hints = [_hint(rs, c0 + bb, g.h, g.tail) for bb in (b2, b1, b2, b1)]
        g.off = off
        off += size
        out.append(g)
    return out


@functools.lru_cache(maxsize=None)
def repair_reference():
    """per case of repair_table(): (ref_fix(...), ref_hop1(... end1)) -- computed once, shared by the tests, never changed"""
    return [(ref_fix(g.t, g.lat, g.mask, g.h, g.tail, g.b, g.dl, g.end), ref_hop1(g.t, g.lat, g.mask, g.h, g.tail, g.b, g.end1))
            for g in repair_table()]


def tie_class(keys):
    """how the minimum of a list of (time, latency) keys is decided: 'time' (one record has the smallest time), 'lat' (several
    share it, the latency decides), 'order' (several share both: the first in ring order); None for an empty list"""
    if not keys:
        return None
    m = min(keys)
    if sum(1 for k in keys if k[0] == m[0]) == 1:
        return "time"
    return "lat" if sum(1 for k in keys if k == m) == 1 else "order"


def hop2_depends_on_b(g):
    """The one way the hop-2 candidate of a family can depend on b.  Every record of the group passes (or dl == 0: nothing that stays
    is past the forward hop); called with b one past the group -- what an exact search returns -- the window takes in the next
    group, whose records may be past the forward hop, and one of them is the candidate; called with a b inside the group the
    window ends with the group and there is none.  A search IS exact when the whole group passes (the predicate is monotone
    there), so the product calls the repair with that first b only."""
    return g.cls == "all" or g.dl == 0.0


def ring_after(g, fx):
    """the whole ring of a case, by position, after the reference's repair fx = ref_fix(...)"""
    t, lat = g.t.copy(), g.lat.copy()
    pos = np.arange(fx[4], fx[5]) & g.mask
    t[pos], lat[pos] = fx[6], fx[7]
    return t, lat
