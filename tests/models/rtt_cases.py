"""The case table of tests/test_rtt_means_cpu.py (which proves its coverage from numpy and the oracle alone) and of
tests/test_rtt_means.py (which runs it through the harness kernel of rtt_means, tests/kernels/rtt_means_harness.hip).

A RING is `size` records of which only .y is ever read: the forward latencies lat0 of accepted packets.  A CASE is a window of a
ring -- `n` records from cursor `frm` on, addressed (frm + k) & (size - 1) -- and a one-way latency dl: the RTT samples are
s = lat0 + dl in float64, and the reference is what the reference env computes from the Python LIST of them,
    mean = np.mean(list(s));  half = n // 2;  inc = np.mean(list(s[half:])) - np.mean(list(s[:half])) if half >= 1 else 0.0.
Many cases share a ring, so a "value set" of a length is a window somewhere else on a ring, or on another ring.

Kinds of rings (the `kind` of a case is its ring's):
  1  a queue that fills and drains: a saw-tooth lat0 over [0.05, 30] plus jitter, dl one of three latencies
  2  exp(U(-8, 4)), twelve binades of magnitudes side by side
  3  every sample equal: the empty queue of DESIGN.md section 2, lat0 == dl, every RTT 2 * dl
  4  dl = 0.0 and whole RTTs in .y, the call of the latency-noise build; one ring of them has a dl eight binades above its lat0
Lengths above 4096 get kinds 1 and 2 only.

Placement.  Rings of 512 records (lengths <= 512) and of 32 768.  The cursors of the device run free in 32 bits (pcc_retire_env.h:
ha[s] is set to the boundary found and only ever masked where a record is addressed; a reset puts it back to 0), so half of the
windows that wrap around their ring do so at a cursor just below 2**32 (a ring's size divides 2**32: the two wraps coincide).
The wrap point -- the index w of the first sample read from record 0 -- is placed, by construction, inside a block of 8 of a
leaf, on a block edge, among a leaf's leftover samples, in the first half, in the second half, and on a chunk edge;
tests/test_rtt_means_cpu.py asserts from the table that each occurred, with every residue mod 8 of frm and of frm + half.

`leaves(n)` restates the SHAPE of np.add.reduce's summation tree (8192-sample chunks; inside a chunk n -> (n/2 rounded down to a
multiple of 8 | rest) until <= 128) for the coverage conditions only: no sum is taken from it -- every reference value is numpy's."""
import functools

import numpy as np

CHUNK = 8192
LEAF = 128
SMALL_RING, BIG_RING = 512, 32768
LENGTHS = sorted(set(range(1, 301)) | {511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 4103, 7688, 7689}
                 | set(range(8184, 8194)) | {8199, 8200, 8320, 8321, 16383, 16384, 16385, 16513, 24577, 30001})
DLS = (0.03, 0.1, 0.2999)
TABLE_SEED = 20


def leaves(n):
    """[(offset, length, depth, path)] of the leaves of np.add.reduce's tree over n samples, left to right; path is the 'L'/'R'
    turns from the chunk's root."""
    out = []

    def walk(off, m, depth, path):
        if m <= LEAF:
            out.append((off, m, depth, path))
            return
        a = m // 2
        a -= a % 8
        walk(off, a, depth + 1, path + "L")
        walk(off + a, m - a, depth + 1, path + "R")

    for c0 in range(0, n, CHUNK):
        walk(c0, min(CHUNK, n - c0), 0, "")
    return out


def wrap_class(n, w):
    """Where the wrap point w (0 < w < n: sample w is the first read from record 0) falls in the whole list's tree: a set of
    'block' (inside a block of 8), 'edge' (between two blocks, or between the blocks and the leftovers, or between two leaves),
    'leftover' (between two leftover samples), 'chunk' (between two chunks), and 'first' / 'second' (half)."""
    out = set()
    for off, m, _, _ in leaves(n):
        if off <= w < off + m:
            o, full = w - off, 8 * (m // 8)
            out.add("edge" if o == 0 or (o <= full and o % 8 == 0) else "block" if o < full else "leftover")
    if w % CHUNK == 0:
        out.add("chunk")
    half = n // 2
    if w < half:
        out.add("first")
    if w > half:
        out.add("second")
    return out


def make_ring(kind, size, variant):
    rs = np.random.RandomState(1000 * kind + 10 * variant + (1 if size == SMALL_RING else 0))
    k = np.arange(size)
    if kind == 1:
        period = 171 if size == SMALL_RING else (2731, 6151)[variant]
        y = 0.05 + 29.95 * (k % period) / (period - 1.0) + rs.uniform(0.0, 1e-3, size)
    elif kind == 2:
        y = np.exp(rs.uniform(-8.0, 4.0, size))
    elif kind == 3:
        y = np.full(size, (0.1, 0.0371)[variant])
    elif variant == 0:    # whole RTTs: (queueing + propagation) * noise, both ways
        y = (0.06 + 3.0 * (k % 997) / 996.0) * rs.uniform(1.0, 1.1, size) + 0.06 * rs.uniform(1.0, 1.1, size)
    else:                 # the return latency (0.4) eight binades above the forward one (~0.0015)
        y = rs.uniform(0.001, 0.002, size) * rs.uniform(1.0, 1.1, size) + 0.4 * rs.uniform(1.0, 1.1, size)
    y = np.ascontiguousarray(y, dtype=np.float64)
    y.setflags(write=False)
    return y


def _sets(n, kind):
    """value sets of a length: enough of kinds 1 and 2 that at least eight show the order of summation (test_rtt_means_cpu.py:
    30 % of random windows do at n = 9, two thirds from n = 72 on)"""
    if kind in (3, 4):
        return 4 if n <= 4096 else 0
    return 8 if n < 9 else 56 if n < 24 else 32 if n < 72 else 16 if n <= 4096 else 12


def _placements(n, size, count, rs):
    """`count` cursors for windows of n records on a ring of `size`: by turns no wrap, and a wrap point of each class the list
    has room for; every other wrapping window sits just below 2**32."""
    lv = leaves(n)
    out = []
    for i in range(count):
        mode = i % 8
        w = None
        if n >= 2 and mode in (1, 2, 3, 5, 6, 7):
            off, m, _, _ = lv[rs.randint(len(lv))]
            nb, nt = m // 8, m % 8
            if mode in (1, 5) and nb >= 1:                     # inside a block of 8
                w = off + 8 * rs.randint(nb) + rs.randint(1, 8)
            elif mode in (2, 6) and (nb >= 2 or (nb >= 1 and off > 0)):   # on a block edge
                w = off + 8 * rs.randint(0 if off > 0 else 1, nb + (1 if nt else 0))
            elif mode == 3 and nt >= 2:                        # between two leftover samples
                w = off + 8 * nb + rs.randint(1, nt)
            elif mode == 7 and n > CHUNK:                      # on a chunk edge
                w = CHUNK * rs.randint(1, (n - 1) // CHUNK + 1)
            if w is None or not 0 < w < n:
                w = rs.randint(1, n)
        if w is None and n > size - 8:     # (no room to choose a residue without wrapping)
            w = rs.randint(1, n) if n >= 2 else None
        if w is None:
            frm = 8 * rs.randint(0, (size - n) // 8 + 1) + i % 8 if n + 8 <= size else 0
            frm = min(frm, size - n)
            if (i // 8) % 2 == 1:
                frm += size * rs.randint(1, (1 << 32) // size)   # a cursor that has been round its ring a few thousand times
        else:
            frm = (size - w) % size
            frm += ((1 << 32) - size) if (i // 2) % 2 else size * rs.randint(0, (1 << 32) // size - 1)
        out.append(frm)
    return out


class Ring(object):
    """y [size] float64; the cases on it as arrays: frm uint32, n uint32, dl float64; kind, variant, size."""

    def __init__(self, kind, size, variant):
        self.kind, self.size, self.variant = kind, size, variant
        self.y = make_ring(kind, size, variant)
        self.frm, self.n, self.dl = [], [], []

    def add(self, frm, n, dl):
        self.frm.append(frm); self.n.append(n); self.dl.append(dl)

    def freeze(self):
        self.frm = np.asarray(self.frm, dtype=np.uint64).astype(np.uint32)
        self.n = np.asarray(self.n, dtype=np.uint32)
        self.dl = np.asarray(self.dl, dtype=np.float64)
        for a in (self.frm, self.n, self.dl):
            a.setflags(write=False)

    def samples(self, i):
        idx = (int(self.frm[i]) + np.arange(int(self.n[i]), dtype=np.int64)) & (self.size - 1)
        return self.y[idx] + self.dl[i]

    def wrap_point(self, i):
        """index of the first sample read from record 0 (None: the window does not wrap)"""
        w = (self.size - (int(self.frm[i]) & (self.size - 1))) % self.size
        return w if 0 < w < int(self.n[i]) else None

    def __len__(self):
        return len(self.n)


@functools.lru_cache(maxsize=None)
def table():
    """-> the rings, each with its cases.  Built once per process; nothing in it may be written to."""
    rs = np.random.RandomState(TABLE_SEED)
    rings = {}
    for kind in (1, 2, 3, 4):
        for variant in (0, 1):
            rings[(kind, BIG_RING, variant)] = Ring(kind, BIG_RING, variant)
        rings[(kind, SMALL_RING, 0)] = Ring(kind, SMALL_RING, 0)
    for n in LENGTHS:
        for kind in (1, 2, 3, 4):
            count = _sets(n, kind)
            n_small = count // 4 if n <= SMALL_RING else 0
            for size, cnt in ((SMALL_RING, n_small), (BIG_RING, count - n_small)):
                for j, frm in enumerate(_placements(n, size, cnt, rs)):
                    ring = rings[(kind, size, j % 2 if size == BIG_RING else 0)]
                    if kind in (1, 2):
                        dl = DLS[rs.randint(len(DLS))]
                    elif kind == 3:
                        dl = float(ring.y[0]) if j % 2 == 0 else float(ring.y[0]) / 3.0   # (every RTT 2 dl; every RTT equal)
                    else:
                        dl = 0.0
                    ring.add(frm, n, dl)
    out = [rings[k] for k in sorted(rings)]
    for r in out:
        r.freeze()
    return tuple(out)


def reference_case(s):
    """(mean, inc) of one case's samples, as the reference env computes them: np.mean of Python lists."""
    n = len(s)
    half = n // 2
    mean = np.mean(list(s))
    inc = np.mean(list(s[half:])) - np.mean(list(s[:half])) if half >= 1 else 0.0
    return float(mean), float(inc)


@functools.lru_cache(maxsize=None)
def references():
    """-> per ring of table(), (mean [cases], inc [cases]) float64, read-only: computed once and shared by every test."""
    out = []
    for r in table():
        m, d = np.empty(len(r)), np.empty(len(r))
        for i in range(len(r)):
            m[i], d[i] = reference_case(r.samples(i))
        m.setflags(write=False); d.setflags(write=False)
        out.append((m, d))
    return tuple(out)


ORDERS = ("shuffled", "sorted", "sparse")


def ordered(ring, order, lanes, block=256):
    """The cases of `ring` as the harness takes them -> (src, frm, n, dl): src[j] is the case in slot j or -1 for a slot
    without samples (n = 0: its group skips the call).
      shuffled  seeded; one slot in nine empty, so that groups that make the call and groups that skip it share wavefronts,
                and a last workgroup that the table only partly fills
      sorted    by length
      sparse    one live group per workgroup, at a position that moves from workgroup to workgroup; the rest empty"""
    k = len(ring)
    if order == "sorted":
        src = np.argsort(ring.n, kind="stable").astype(np.int64)
    elif order == "shuffled":
        rs = np.random.RandomState(77 + ring.kind + ring.size)
        size = k + k // 8 + 3
        src = np.full(size + (1 if size % (block // 16) == 0 else 0), -1, dtype=np.int64)
        src[rs.permutation(src.size)[:k]] = rs.permutation(k)
    else:
        per = block // lanes
        src = np.full(k * per, -1, dtype=np.int64)
        src[np.arange(k) * per + (np.arange(k) * 5) % per] = np.arange(k)
    live = src >= 0
    frm = np.where(live, ring.frm[np.maximum(src, 0)], np.uint32(0xDEADBEE0)).astype(np.uint32)
    n = np.where(live, ring.n[np.maximum(src, 0)], 0).astype(np.uint32)
    dl = np.where(live, ring.dl[np.maximum(src, 0)], np.nan)
    return src, frm, n, dl
