"""The reference side of tests/test_rtt_means.py and tests/test_rtt_lengths.py, proved on the CPU from numpy and the C oracle
alone: no device code is involved in anything this file asserts.

  1. the case table (tests/models/rtt_cases.py): the oracle's np_mean -- the routine every simulator parity test leans on --
     gives numpy's bits on every case; the table reaches every edge of np.add.reduce's summation tree that rtt_means
     (pcc-rl_amd/csrc/pcc_retire_env.h) has a line of code for; and its values SHOW the order of summation: a kernel that
     summed left to right would differ from numpy on them.
  2. the link families of tests/test_rtt_lengths.py, which drive the product's own kernels to those lengths: what lengths
     (acknowledgements per interval) the oracle reaches on each, and that the deep-queue family fits the rings.

On "depth 7 on a left-most and a right-most path": a left part is a multiple of 8 and at most half of its parent, and everything
under a multiple of 8 <= 4096 splits evenly, so no leaf under ANY left part is deeper than the left-most leaf of a full chunk
(depth 6): the only depth-7 leaves a chunk can have are the two at the bottom of its right spine, RRRRRRL and RRRRRRR (asserted
below over every n of a chunk).  The table is held to both of them -- the left one is fed with seven sums' slots open, the right
one pops all seven -- in a first chunk and in a later one (the running total is not zero then)."""
import functools
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import rtt_cases as rc   # noqa: E402

RING_CAPACITY = 32768      # pcc_rl_amd.env.DEFAULT_RING_CAPACITY: records of a sender's accepted ring (the dropped ring: twice that)


# ------------------------------------------------------------------------------------------------ 1. the table
def test_oracle_np_mean_is_numpy_on_every_case():
    """ties the table to the oracle the simulator tests compare with: mean and both halves, every case"""
    for ring, (mean, inc) in zip(rc.table(), rc.references()):
        for i in range(len(ring)):
            s = ring.samples(i)
            half = len(s) // 2
            assert oracle.np_mean(s) == mean[i], (ring.kind, ring.size, i)
            want = oracle.np_mean(s[half:]) - oracle.np_mean(s[:half]) if half >= 1 else 0.0
            assert want == inc[i] and np.isfinite(mean[i]) and np.isfinite(inc[i]), (ring.kind, ring.size, i)


def test_lengths_of_the_table():
    want = set(range(1, 301)) | {511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 4103, 7688, 7689, 8184, 8185, 8186,
                                 8187, 8188, 8189, 8190, 8191, 8192, 8193, 8199, 8200, 8320, 8321, 16383, 16384, 16385, 16513, 24577, 30001}
    assert set(rc.LENGTHS) == want
    kinds = {}
    for ring in rc.table():
        assert ring.size in (rc.SMALL_RING, rc.BIG_RING) and ring.y.shape == (ring.size,)
        assert ring.size == rc.BIG_RING or ring.n.max() <= rc.SMALL_RING      # the small ring: n <= 512 only
        assert (ring.n <= ring.size).all() and (ring.n >= 1).all()
        for n in np.unique(ring.n):
            kinds.setdefault(int(n), set()).add(ring.kind)
    assert set(kinds) == want
    for n, k in kinds.items():
        assert k == ({1, 2, 3, 4} if n <= 4096 else {1, 2}), (n, k)
    # kind 3: every sample of a case equal; kind 4: dl == 0.0, and one ring whose samples sit eight binades above their spread
    for ring in rc.table():
        if ring.kind == 3:
            assert (ring.y == ring.y[0]).all()
        if ring.kind == 4:
            assert (ring.dl == 0.0).all()
        else:
            assert (ring.dl > 0.0).all()
    far = [r for r in rc.table() if r.kind == 4 and r.variant == 1]
    assert far and all(0.4 <= r.y.min() and r.y.max() < 0.4 * 1.1 + 0.0025 for r in far)     # 0.4 s back, 0.001..0.0022 s forth


def test_the_table_reaches_every_edge_of_the_summation_tree():
    lengths = rc.LENGTHS
    depths, leaf_lens, chunk_counts, last_chunks = set(), set(), set(), set()
    deep = set()
    for n in lengths:
        lv = rc.leaves(n)
        assert sum(m for _, m, _, _ in lv) == n and all(0 < m <= 128 for _, m, _, _ in lv)
        chunk_counts.add(-(-n // rc.CHUNK))
        last = n - (n - 1) // rc.CHUNK * rc.CHUNK
        if n > rc.CHUNK:
            last_chunks.add("<8" if last < 8 else "8..128" if last <= 128 else ">128")
        for off, m, d, path in lv:
            depths.add(d)
            leaf_lens.add(m)
            if d == 7:
                deep.add((path, off >= rc.CHUNK))
            assert d <= 7, (n, d)          # kWalkDepth: the walk's stack has seven levels and no more is ever needed
    assert depths == set(range(8))
    assert max(d for _, _, d, _ in rc.leaves(7688)) == 6 and max(d for _, _, d, _ in rc.leaves(7689)) == 7     # where depth 7 begins
    # every leaf of every n of a chunk: seven levels, never eight, and the seventh only at the bottom of the right spine
    every = {(d, path) for n in range(1, rc.CHUNK + 1) for _, _, d, path in rc.leaves(n) if d >= 7}
    assert every == {(7, "RRRRRRL"), (7, "RRRRRRR")}
    assert deep == {(p, later) for p in ("RRRRRRL", "RRRRRRR") for later in (False, True)}
    assert {m % 8 for m in leaf_lens if 8 <= m <= 128} == set(range(8)) and {8, 128} <= leaf_lens
    assert set(range(8, 129)) <= leaf_lens          # (every leaf length, in fact)
    assert chunk_counts == {1, 2, 3, 4}
    assert last_chunks == {"<8", "8..128", ">128"}
    # the halves: which of (first, second) is a single short leaf decides whether they share a call
    pairs = {(n // 2, n - n // 2) for n in lengths if n >= 2}
    assert {(71, 71), (71, 72), (72, 72), (72, 73)} <= pairs
    combos = {(a < 72, b < 72) for a, b in pairs}
    assert combos == {(True, True), (True, False), (False, False)}     # (second < 72 <= first cannot be: second >= first)


def test_placements_of_the_table():
    frm_res, half_res, wraps, high, sizes = set(), set(), {}, 0, set()
    for ring in rc.table():
        sizes.add(ring.size)
        for i in range(len(ring)):
            n, frm = int(ring.n[i]), int(ring.frm[i])
            frm_res.add((ring.size, frm % 8))
            half_res.add((ring.size, (frm + n // 2) % 8))
            w = ring.wrap_point(i)
            if w is not None:
                for c in rc.wrap_class(n, w):
                    wraps[(ring.size, c)] = wraps.get((ring.size, c), 0) + 1
                if frm + n > 1 << 32:
                    high += 1
                    assert frm >= (1 << 32) - ring.size         # the cursor itself wraps in its 32 bits inside the window
    assert sizes == {rc.SMALL_RING, rc.BIG_RING}
    assert frm_res == {(s, r) for s in sizes for r in range(8)} and half_res == frm_res
    for size in sizes:
        for c in ("block", "edge", "leftover", "first", "second"):
            assert wraps.get((size, c), 0) >= 20, (size, c, wraps)
    assert wraps.get((rc.BIG_RING, "chunk"), 0) >= 8, wraps
    assert high >= 500
    # per length, too: every length from 9 up has windows that wrap and windows that do not
    wrapped, straight = set(), set()
    for ring in rc.table():
        for i in range(len(ring)):
            (straight if ring.wrap_point(i) is None else wrapped).add(int(ring.n[i]))
    assert {n for n in rc.LENGTHS if n >= 9} <= wrapped and {n for n in rc.LENGTHS if n >= 9} <= straight


ORDER_CLASSES = ((9, 71), (72, 128), (129, 4096), (4097, 8192), (8193, 1 << 30))


def test_the_values_show_the_order_of_summation():
    """A condition on the inputs (no code under test is involved): over the cases of kinds 1 and 2 with n >= 9, a plain
    left-to-right sum (np.cumsum adds in order) differs from np.mean
      * in at least a quarter of the cases of every length class -- the classes are the routine's own: short leaves that may share a
        call (< 72), the wide leaf (72..128), trees inside one chunk up to and past 4096, several chunks;
      * and in at least eight cases of every single length.
    A quarter of every single length cannot be had from ANY values: for n = 11..15 numpy's order and the plain one differ only in how
    the first eight samples are folded, and the following plain adds round most of those differences away -- 19 to 23 % of random
    value sets show it there whatever their distribution (U(1, 2), exp(U(-8, 4)), a ramp with jitter; 4 000 sets each), 30 % at
    n = 9, a half from n = 16 on.  Hence the many value sets of the lengths below 24 (tests/models/rtt_cases.py: _sets)."""
    shown, total = {}, {}
    for ring, (mean, _) in zip(rc.table(), rc.references()):
        if ring.kind not in (1, 2):
            continue
        for i in range(len(ring)):
            n = int(ring.n[i])
            if n < 9:
                continue
            s = ring.samples(i)
            total[n] = total.get(n, 0) + 1
            shown[n] = shown.get(n, 0) + (np.cumsum(s)[-1] / n != mean[i])
    assert set(total) == {n for n in rc.LENGTHS if n >= 9}
    worst = min(total, key=lambda n: shown[n] / total[n])
    print("order shown: worst single length %.2f at n = %d; fewest cases of a length %d" % (shown[worst] / total[worst], worst, min(shown.values())))
    for n in total:
        assert shown[n] >= 8, (n, shown[n], total[n])
    for lo, hi in ORDER_CLASSES:
        sh, tot = (sum(v for n, v in d.items() if lo <= n <= hi) for d in (shown, total))
        print("  lengths %d..%d: %d of %d cases" % (lo, min(hi, max(total)), sh, tot))
        assert tot > 0 and sh >= 0.25 * tot, (lo, hi, sh, tot)
    assert shown[9] >= 0.25 * total[9] and shown[17] >= 0.25 * total[17] and all(shown[n] >= 0.25 * total[n] for n in total if n >= 72)


def test_a_quarter_of_a_single_length_is_out_of_reach_at_11_to_15_samples():
    """Why the floor above is per class: for n = 11..15, whatever the values are drawn from, fewer than a quarter of random value
    sets tell numpy's order from the plain one (1 500 sets per length and distribution; a fifth, give or take, do) -- while at
    n = 9 and from n = 16 on more than a quarter do."""
    rs = np.random.RandomState(5)
    draws = {"U(1, 2)": lambda n: rs.uniform(1.0, 2.0, n), "exp(U(-8, 4)) + 0.1": lambda n: np.exp(rs.uniform(-8.0, 4.0, n)) + 0.1,
             "a level with jitter": lambda n: rs.uniform(0.05, 30.0) + rs.uniform(0.0, 1e-3, n) + 0.1}
    sets = 1500
    for name, draw in draws.items():
        share = {}
        for n in (9, 11, 12, 13, 14, 15, 16):
            share[n] = sum(np.cumsum(s)[-1] / n != np.mean(list(s)) for s in (draw(n) for _ in range(sets))) / sets
        print("%s: %s" % (name, {n: round(v, 3) for n, v in share.items()}))
        assert all(0.12 < share[n] < 0.25 for n in (11, 12, 13, 14, 15)), (name, share)
        assert share[9] > 0.25 and share[16] > 0.4, (name, share)


def test_orderings_present_every_case_once():
    for ring in rc.table():
        for lanes in (8, 16):
            for order in rc.ORDERS:
                src, frm, n, dl = rc.ordered(ring, order, lanes)
                live = src >= 0
                assert np.array_equal(np.sort(src[live]), np.arange(len(ring)))
                assert (n[~live] == 0).all() and np.array_equal(n[live], ring.n[src[live]]) and np.array_equal(frm[live], ring.frm[src[live]])
                per = 256 // lanes
                if order == "sparse":
                    assert src.size == len(ring) * per and (live.reshape(-1, per).sum(axis=1) == 1).all()
                if order == "sorted":
                    assert (np.diff(n.astype(np.int64)) >= 0).all()
                if order == "shuffled":
                    assert (~live).sum() >= len(ring) // 9 and src.size % per != 0     # (the last workgroup: groups past the table's end)


# ------------------------------------------------------------------------------------------------ 2. the link families
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def lengths_of(ref, first_step=0):
    """acknowledgements per interval, the oracle's `acked` column: the n of every rtt_means call"""
    return ref["steps"][..., first_step:, 1].astype(np.int64)


def histogram(lengths):
    """for the record under profiles/: counts per class of lengths"""
    edges = [0, 1, 9, 72, 129, 273, 513, 1025, 2049, 4097, 7689, 8193, 8321, 16385, 1 << 30]
    h = np.histogram(np.asarray(lengths).ravel(), bins=edges)[0]
    return {"%d..%d" % (edges[k], edges[k + 1] - 1) if k + 2 < len(edges) else ">=%d" % edges[k]: int(h[k]) for k in range(len(h))}


def fits_the_rings(ref, links):
    """Per env of a one-sender batch on links WITHOUT random loss: do its rings (pcc_dev.h: an accepted ring of ring_capacity records,
    a dropped ring of twice that) hold every record between a send half and the retire half after it?  From the oracle's columns and
    the links.  With U = packets under way at an interval's end (the warm-up's -- heap length less the pending SEND -- + sent - acked
    - lost since), A of them accepted:
      accepted ring after the send half of interval t = A(start) + accepted SENDs of t = A(end) + acked(t), and the link bounds A: at
        most queue + 1 packets in the queue and bw * dl + 1 on each of the two legs;
      dropped ring = (U - A)(start) + dropped SENDs of t = U(end) - A(end) + lost(t) <= U(end) + lost(t)."""
    sent, acked, lost = (ref["steps"][..., c].astype(np.int64) for c in (0, 1, 2))
    assert (links[:, 3] == 0.0).all()
    under_way = (ref["warm"][:, 1].astype(np.int64) - 1)[:, None] + np.cumsum(sent - acked - lost, axis=1)
    accepted = links[:, 2] + 2.0 * links[:, 0] * links[:, 1] + 3.0
    return (accepted + acked.max(axis=1) <= RING_CAPACITY) & ((under_way + lost).max(axis=1) + 2 <= 2 * RING_CAPACITY)


D_ENVS, D_STEPS, D_SEED = 48, 40, 3


def deep_links():
    """Family D's links and its RandomState, drawn in the order bw, dl, queue: 48 fixed links whose queues hold 16 500 to 19 000
    packets, sent into at the maximum rate: once a queue is full an interval is half of (queue / bw + 2 dl) long and brings about
    queue / 2 acknowledgements, whatever the actions do above the bandwidth."""
    rs = np.random.RandomState(1)
    bw, dl, q = rs.uniform(380, 520, D_ENVS), rs.uniform(0.03, 0.3, D_ENVS), rs.uniform(16500, 19000, D_ENVS)
    return np.stack([bw, dl, q, np.zeros(D_ENVS), np.full(D_ENVS, 1000.0)], axis=1), rs


@functools.lru_cache(maxsize=None)
def family_d(features=oracle.DEFAULT_FEATURES):
    params, rs = deep_links()
    acts = rs.uniform(-2, 2, (D_ENVS, D_STEPS))
    ref = oracle.run_batch(acts, seed=D_SEED, params=params, features=features, n_threads=8)
    return _frozen(dict(acts=acts, links=params, seed=D_SEED, fits=fits_the_rings(ref, params), **{k: v for k, v in ref.items() if v is not None}))


@functools.lru_cache(maxsize=None)
def depth_of(n):
    """the deepest leaf of np.add.reduce's tree over n samples: how many levels of the walk's stack the list fills"""
    return max(d for _, _, d, _ in rc.leaves(n)) if n > 0 else 0


def assert_deep_lengths(ref, fits, what=""):
    """Family D's conditions on the oracle's lengths: every env (that fits the rings) has an interval >= 7689 and one past the chunk
    edge (> 8192); the batch reaches both sides of 8192 + 128, where the last chunk stops being one leaf.  This is the CHUNK family:
    a list past 8192 is a full chunk (8192 -> ... -> 128: six levels) and a remainder below 1 400 (four), so none of ITS long
    lists fills the seventh level -- that takes a chunk of 7689..8191 samples, which this family only passes through on the way
    up (asserted: some env does).  Family E is the one that stays there."""
    n = lengths_of(ref)[fits]
    assert fits.sum() >= 40, (what, fits.sum())
    assert ((n >= 7689).any(axis=1) & (n > 8192).any(axis=1)).all(), what
    over = n[n > 8192]
    assert (over <= 8192 + 128).any() and (over > 8192 + 128).any(), what
    assert all(depth_of(int(v)) <= 6 for v in np.unique(over)), what
    assert ((n >= 7689) & (n <= 8192)).any(), what
    return n


E_SEED = 3


def edge_links():
    """Family E: family D's links with queues of 15 350 to 16 150 packets (RandomState(5), the same order of draws): full, they
    bring 7 700 to 8 165 acknowledgements an interval -- one chunk, seven levels deep unless the count is a multiple of 8 (a full
    queue can hold an env at one length for many steps: the draws are chosen so that no env sits on such a length)."""
    rs = np.random.RandomState(5)
    bw, dl, q = rs.uniform(380, 520, D_ENVS), rs.uniform(0.03, 0.3, D_ENVS), rs.uniform(15350, 16150, D_ENVS)
    return np.stack([bw, dl, q, np.zeros(D_ENVS), np.full(D_ENVS, 1000.0)], axis=1), rs


@functools.lru_cache(maxsize=None)
def family_e(features=oracle.DEFAULT_FEATURES):
    params, rs = edge_links()
    acts = rs.uniform(-2, 2, (D_ENVS, D_STEPS))
    ref = oracle.run_batch(acts, seed=E_SEED, params=params, features=features, n_threads=8)
    return _frozen(dict(acts=acts, links=params, seed=E_SEED, fits=fits_the_rings(ref, params), **{k: v for k, v in ref.items() if v is not None}))


def assert_seventh_level(ref, fits, what=""):
    """Family E's condition on the oracle's lengths: every env (that fits the rings) has at least three lists whose tree is seven
    levels deep (counted with depth_of, not assumed from 7689 <= n <= 8192: 8184 and 8192 are six deep), and no list reaches the
    chunk edge."""
    n = lengths_of(ref)[fits]
    assert fits.sum() >= 40, (what, fits.sum())
    deep = np.vectorize(depth_of)(n) == 7
    assert (deep.sum(axis=1) >= 3).all(), (what, deep.sum(axis=1).min())
    assert n.max() <= 8192, (what, n.max())
    return n


def test_family_e_fills_the_seventh_level_in_every_env():
    c = family_e()
    n = assert_seventh_level(c, c["fits"])
    deep = np.vectorize(depth_of)(n) == 7
    print("family E: %d of %d envs fit; lists seven levels deep per env %d..%d, %d in all; longest list %d; %s"
          % (c["fits"].sum(), D_ENVS, deep.sum(axis=1).min(), deep.sum(axis=1).max(), deep.sum(), n.max(), histogram(n)))
    assert c["fits"].all()
    assert depth_of(7688) == 6 and depth_of(7689) == 7 and depth_of(8191) == 7 and depth_of(8192) == 6 and depth_of(9568) == 6
    c2 = family_e(("send ratio", "latency ratio"))
    assert np.array_equal(c2["steps"], c["steps"])


def test_family_d_reaches_the_chunk_edge_and_fits_the_rings():
    c = family_d()
    n = assert_deep_lengths(c, c["fits"])
    top = n.max(axis=1)
    print("family D: %d of %d envs fit; per-env longest list %d..%d; %s" % (c["fits"].sum(), D_ENVS, top.min(), top.max(), histogram(n)))
    assert c["fits"].all() and top.min() == 8267 and top.max() == 9568       # (frozen: what the C oracle gives on these draws)
    assert not (c["steps"][..., 2] > c["steps"][..., 0]).any()
    # the same family under the two-feature observation of the need_halves == false route: the same lengths
    c2 = family_d(("send ratio", "latency ratio"))
    assert np.array_equal(c2["steps"], c["steps"])


S_ENVS, S_STEPS, S_SEED = 512, 60, 31


def short_links(n_senders=1, seed=S_SEED, n=S_ENVS):
    """Family S's links: starting rates over [40, 1000] (half of them log-uniform), latencies over [0.01, 0.6], the bandwidth a
    little below or a little above the rate, queues of 1 to 59 packets, random loss up to 0.3 and 1.0 on six envs; every eighth
    env a queue of 200 to 1 500 and every sixteenth a fast, long link with a queue of 800 to 2 500 for the lengths past 512."""
    rs = np.random.RandomState(seed)
    k = np.arange(n)
    rate0 = np.where(k % 2 == 0, np.exp(rs.uniform(np.log(40), np.log(1000), n)), rs.uniform(40, 1000, n))
    dl = np.where(k % 4 < 2, np.exp(rs.uniform(np.log(0.01), np.log(0.6), n)), rs.uniform(0.01, 0.6, n))
    bw = rate0 * np.where(rs.randint(2, size=n) == 0, rs.uniform(0.8, 0.98, n), rs.uniform(1.02, 1.3, n))
    q = np.where(k % 8 == 7, rs.randint(200, 1500, n), rs.randint(1, 60, n)).astype(float)
    loss = rs.uniform(0, 0.3, n)
    loss[rs.permutation(n)[:6]] = 1.0
    deep = k % 16 == 15
    rate0 = np.where(deep, rs.uniform(700, 1000, n), rate0)
    dl = np.where(deep, rs.uniform(0.3, 0.6, n), dl)
    q = np.where(deep, rs.randint(800, 2500, n), q).astype(float)
    bw = np.where(deep, rate0 * rs.uniform(0.8, 0.98, n), bw)
    loss = np.where(deep, rs.uniform(0, 0.03, n), loss)
    cols = [bw, dl, q, loss, rate0] + ([np.clip(rate0 * rs.uniform(0.5, 1.5, n), 40.0, 1000.0)] if n_senders == 2 else [])
    return np.stack(cols, axis=1), rs


@functools.lru_cache(maxsize=None)
def family_s(features=oracle.DEFAULT_FEATURES, n_senders=1, latency_noise=None, n=S_ENVS, steps=S_STEPS):
    params, rs = short_links(n_senders, n=n)
    acts = rs.uniform(-1, 1, (n, steps) if n_senders == 1 else (n, steps, 2))
    ref = oracle.run_batch(acts, n_senders=n_senders, seed=S_SEED, params=params, features=features, latency_noise=latency_noise, n_threads=8)
    return _frozen(dict(acts=acts, links=params, seed=S_SEED, **{k: v for k, v in ref.items() if v is not None}))


def assert_short_lengths(ref, what=""):
    """Family S's conditions: every length 0..272 at least three times at steps >= 1, and lengths in (272, 512], (512, 1024] and
    (1024, 2048]."""
    n = lengths_of(ref, 1).ravel()
    h = np.bincount(n, minlength=273)
    assert h[:273].min() >= 3, (what, int(h[:273].argmin()), int(h[:273].min()))
    for lo, hi in ((272, 512), (512, 1024), (1024, 2048)):
        assert ((n > lo) & (n <= hi)).any(), (what, lo, hi)
    return n


def test_family_s_reaches_every_short_length():
    c = family_s()
    n = assert_short_lengths(c)
    print("family S: every length 0..272 at least %d times; longest %d; %s" % (np.bincount(n, minlength=273)[:273].min(), n.max(), histogram(n)))
    assert (c["links"][:, 3] == 1.0).sum() == 6 and (c["steps"][c["links"][:, 3] == 1.0][..., 1] == 0).all()    # loss 1.0: no list at all
    c2 = family_s(("send ratio", "latency ratio"))
    assert np.array_equal(c2["steps"], c["steps"])


# what the oracle shows the other routes of tests/test_rtt_lengths.py reach (asserted there from the same dictionaries; the floors
# below are what two senders on one bottleneck, and the event loop inside ring_capacity events, can produce on family S's links)
TWO_SENDER_FLOOR = (200, 3)      # every per-sender length 0..200 at least three times (the slower sender's first gap: 238)
NOISE_ENVS, NOISE_STEPS = 256, 40


def assert_two_sender_lengths(ref):
    n = ref["steps"][..., 1:, 1].astype(np.int64)          # [envs, senders, steps]
    for s in range(2):
        h = np.bincount(n[:, s].ravel(), minlength=TWO_SENDER_FLOOR[0] + 1)
        assert h[:TWO_SENDER_FLOOR[0] + 1].min() >= TWO_SENDER_FLOOR[1], (s, int(h[:TWO_SENDER_FLOOR[0] + 1].argmin()))
        assert (n[:, s] > 512).any(), s
    # the two lists of an env differ in length in most intervals: the senders' calls are not in step
    assert (n[:, 0] != n[:, 1]).mean() > 0.5
    return n


def assert_noise_lengths(ref):
    n = lengths_of(ref, 1).ravel()
    assert (n > 128).sum() >= 100 and (n > 1024).sum() >= 20
    assert set(range(0, 129)) <= set(n.tolist())
    return n


def test_two_sender_and_noise_families():
    c = family_s(n_senders=2)
    n = assert_two_sender_lengths(c)
    print("family S, two senders: per-sender longest %s; %s" % (n.max(axis=(0, 2)), histogram(n)))
    c = family_s(latency_noise=1.1, n=NOISE_ENVS, steps=NOISE_STEPS)
    n = assert_noise_lengths(c)
    sent = c["steps"][..., 0]
    print("family S, latency noise 1.1: longest %d (longest interval %d SENDs); %s" % (n.max(), sent.max(), histogram(n)))
    assert sent.max() + n.max() < RING_CAPACITY
