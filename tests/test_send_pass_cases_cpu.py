"""The reference side of tests/test_send_pass_device.py, proved on the CPU from the case tables of tests/models/send_pass_cases.py
and the CPU models alone: no device code is involved in anything this file asserts.

  1. the reference has a second witness: the C recurrence the tables are held to (serial_mi / the merged `plain`, through
     pcc_cases_plain / pcc_cases2_plain) equals a dozen-line restatement of ns:66-84 written here, on a few hundred small cases.
  2. the mirrors (model_mi; the token and sweep passes of two senders) equal the plain recurrence bit for bit on EVERY case of
     every table: the per-case counts below come from passes that are exact.
  3. coverage: every class (c) to (k) has at least FLOOR cases, and where a class names a regime or a refusal cause the mirror's
     per-case counts show that at least FLOOR cases take it: the tie that runs and the tie that refuses (and regime C's), the cut
     by the top of t's binade at every lane position and in every wavefront, free mode on each side of its margin, a token
     shortage that starts at each listed lane (every position of it).  The floor is a cap on how thin a table may be, not a
     measurement: a table that does not meet it is changed until it does.
  4. every case passes the harness's own validation rules, restated in send_pass_cases.py, stays within the packet limit, and
     the arenas stay below 1 GB."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import send_pass_cases as sc   # noqa: E402

FLOOR = 50
LANES = (64, 256)


# ------------------------------------------------------------------------------------------------ 1. a second witness
def py_recurrence(q, tu, t, dl, maxq, ebw, gap, end, loss):
    """Link.packet_enters_link and the sender's clock, ns:66-84, 161, 170-175, one SEND after the other"""
    acc, drp, k = [], [], 0
    while t < end:
        qcur = max(0.0, q - (t - tu))        # ns:66-67: the queue drained to now
        lat = dl + qcur                      # ns:170
        rec = (t + lat, lat)                 # ns:174, 173
        if loss[k]:                          # ns:73-74: lost at random, the link is not touched
            drp.append(rec)
        else:
            q, tu = qcur, t                  # ns:75-76
            if ebw + q > maxq:               # ns:79-81: the queue is full
                drp.append(rec)
            else:
                q = q + ebw                  # ns:82
                acc.append(rec)
        t += gap                             # ns:161
        k += 1
    return q, tu, t, acc, drp


def bits(x):
    """a float64 as its 64 bits: -0.0 is not +0.0"""
    return int(np.float64(x).view(np.int64))


def small_cases(tab, limit=500, count=120):
    idx = np.flatnonzero(tab.npk <= limit)
    return idx[:: max(1, len(idx) // count)][:count]


@pytest.mark.parametrize("name", ["c", "d", "e", "g", "j"])
def test_c_recurrence_equals_python_restatement(name):
    tab = sc.CLASSES1[name](64)
    idx = small_cases(tab)
    assert len(idx) >= 60
    for c in idx:
        f, o = tab.f, int(tab.off[c])
        q, tu, t, acc, drp = py_recurrence(f["q"][c], f["tu"][c], f["t"][c], f["dl"][c], f["maxq"][c], f["ebw"][c], f["gap"][c], f["end"][c],
                                           tab.loss[o:])
        r = tab.ref[c]
        assert (bits(q), bits(tu), bits(t), len(acc), len(drp)) == (bits(r["q"]), bits(r["tu"]), bits(r["t"]), r["na"], r["nd"]), (name, c)
        assert np.array_equal(np.array(acc, dtype=np.float64).reshape(-1, 2).view(np.int64),
                              np.stack([tab.acc["t1"][o:o + len(acc)], tab.acc["lat"][o:o + len(acc)]], axis=1).view(np.int64)), (name, c)
        assert np.array_equal(np.array(drp, dtype=np.float64).reshape(-1, 2).view(np.int64),
                              np.stack([tab.drp["t1"][o:o + len(drp)], tab.drp["lat"][o:o + len(drp)]], axis=1).view(np.int64)), (name, c)


def py_recurrence2(q, tu, t, dl, maxq, ebw, gap, end, loss):
    """two senders on the link: the earlier SEND first, sender 0 on equal times"""
    t = list(t)
    acc, drp, k = ([], []), ([], []), 0
    while min(t) < end:
        s = 1 if t[1] < t[0] else 0
        qcur = max(0.0, q - (t[s] - tu))
        lat = dl + qcur
        rec = (t[s] + lat, lat)
        if loss[k]:
            drp[s].append(rec)
        else:
            q, tu = qcur, t[s]
            if ebw + q > maxq:
                drp[s].append(rec)
            else:
                q = q + ebw
                acc[s].append(rec)
        t[s] += gap[s]
        k += 1
    return q, tu, t, acc, drp


def test_c_merged_recurrence_equals_python_restatement():
    tab = sc.CLASSES2["k_pairs_trace"]()
    idx = small_cases(tab, limit=1000, count=100)
    assert len(idx) >= 60
    for c in idx:
        f, o = tab.f, int(tab.off[c])
        q, tu, t, acc, drp = py_recurrence2(f["q"][c], f["tu"][c], f["t"][c], f["dl"][c], f["maxq"][c], f["ebw"][c], f["gap"][c], f["end"][c],
                                            tab.loss[o:])
        r = tab.ref[c]
        assert (bits(q), bits(tu), bits(t[0]), bits(t[1])) == (bits(r["q"]), bits(r["tu"]), bits(r["t"][0]), bits(r["t"][1])), c
        for s in range(2):
            assert (len(acc[s]), len(drp[s])) == (r["a"][s], r["d"][s]), (c, s)
            for got, recs in ((acc[s], tab.recs[2 * s]), (drp[s], tab.recs[2 * s + 1])):
                want = np.stack([recs["t1"][o:o + len(got)], recs["lat"][o:o + len(got)]], axis=1)
                assert np.array_equal(np.array(got, dtype=np.float64).reshape(-1, 2).view(np.int64), want.view(np.int64)), (c, s)


# ------------------------------------------------------------------------------------------------ 2, 4: every table
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", sorted(sc.CLASSES1))
def test_one_sender_table(name, lanes):
    tab = sc.CLASSES1[name](lanes)
    counts, same = tab.mirror()
    assert same, "the mirror differs from the plain recurrence"
    # the mirror sends every packet by some pass
    assert (counts[:, [sc.PK_A, sc.PK_BSCAN, sc.PK_BFREE, sc.PK_C, sc.PK_S, sc.PK_CHAIN]].sum(axis=1) == tab.npk).all()
    if lanes == 256:
        assert counts[:, sc.PK_C].sum() == 0          # a team pass has no regime C
    # (4) validation, restated; the packet limit; the arena
    limit = sc.MAX_PACKETS if lanes == 64 else sc.TEAM_MAX_PACKETS
    assert tab.arena_records < (1 << 26)
    assert int(tab.npk.max()) <= limit
    f = tab.f
    for c in range(tab.n):
        assert sc.valid_clock(f["t"][c], f["gap"][c], f["end"][c], limit), (name, c)
        assert sc.valid_ring(tab.arena_records, int(tab.ring_off[c]), int(tab.cap[c])), (name, c)
        assert all(np.isfinite(f[k][c]) for k in ("q", "tu", "dl", "lr", "maxq", "ebw")), (name, c)
        if tab.trace:
            assert tab.trace_off[c] >= 0 and tab.trace_stride[c] >= 0 and tab.trace_off[c] + tab.trace_stride[c] <= len(tab.trace_arr), (name, c)
    # rings do not overlap
    order = np.argsort(tab.ring_off)
    assert (tab.ring_off[order][1:] >= tab.ring_off[order][:-1] + 3 * tab.cap[order][:-1]).all()
    if not name.startswith("i"):
        assert (tab.cap >= np.maximum(tab.ref["na"], (tab.ref["nd"] + 1) // 2)).all()     # every record is kept (but in class i)


@pytest.mark.parametrize("name", sorted(sc.CLASSES2))
def test_two_sender_table(name):
    tab = sc.CLASSES2[name]()
    counts, same = tab.mirror()
    assert same, "the mirror differs from the plain merged recurrence"
    assert (counts[:, [1, 3, 5, 7]].sum(axis=1) == tab.npk).all()
    assert tab.arena_records < (1 << 26)
    f = tab.f
    na, nd = tab.ref["a"].astype(np.int64), tab.ref["d"].astype(np.int64)
    assert int((na + nd).max()) <= sc.MAX_PACKETS
    for c in range(tab.n):
        for s in range(2):
            assert sc.valid_clock(f["t"][c, s], f["gap"][c, s], f["end"][c], sc.MAX_PACKETS), (name, c)
            assert sc.valid_ring(tab.arena_records, int(tab.ring_off[c, s]), int(tab.cap[c, s])), (name, c)
        if tab.trace:
            assert tab.trace_off[c] + tab.trace_stride[c] <= len(tab.trace_arr)
    flat_off, flat_cap = tab.ring_off.reshape(-1), tab.cap.reshape(-1)
    assert (flat_off[1:] >= flat_off[:-1] + 3 * flat_cap[:-1]).all()


# ------------------------------------------------------------------------------------------------ 3. coverage
def n_where(tab, counts, sub, cond):
    return int(((tab.sub == sub) & cond).sum())


@pytest.mark.parametrize("lanes", LANES)
def test_every_class_has_its_cases(lanes):
    for name in sorted(sc.CLASSES1):
        assert sc.CLASSES1[name](lanes).n >= FLOOR, name
    for name in sorted(sc.CLASSES2):
        assert sc.CLASSES2[name]().n >= FLOOR, name


@pytest.mark.parametrize("lanes", LANES)
def test_ties_run_and_refuse(lanes):
    tab = sc.ties(lanes)
    counts, _ = tab.mirror()
    assert n_where(tab, counts, "even", (counts[:, sc.TIE_RUN] > 0) & (counts[:, sc.TIE_REFUSED] == 0)) >= FLOOR     # the pass runs
    assert n_where(tab, counts, "odd", counts[:, sc.TIE_REFUSED] > 0) >= FLOOR                                       # it refuses
    if lanes == 64:
        assert n_where(tab, counts, "ctie", (counts[:, sc.C_TIE_REFUSED] > 0) & (counts[:, sc.PK_C] == 0)) >= FLOOR


@pytest.mark.parametrize("lanes", LANES)
def test_binade_top_cuts_at_every_position(lanes):
    tab = sc.time_edges(lanes)
    counts, _ = tab.mirror()
    top = (tab.sub == "top") & (counts[:, sc.TOP_CUT] > 0)
    assert top.sum() >= FLOOR
    pos = counts[top, sc.TOP_POS] - 1
    for i in range(4):
        for w in range(lanes // 64):
            assert ((pos % 4 == i) & (pos // 256 == w)).sum() >= 3, (i, w)
    # ... by every closed-form regime
    for col in (sc.PK_A, sc.PK_BSCAN, sc.PK_BFREE):
        assert (top & (counts[:, col] > 0)).sum() >= FLOOR // 2
    # the other edges: what they say they are
    assert (tab.npk[tab.sub == "none"] == 0).all() and (tab.sub == "none").sum() >= FLOOR
    assert (tab.npk[tab.sub == "one"] == 1).all() and (tab.sub == "one").sum() >= FLOOR
    assert set(tab.npk[tab.sub == "lane0"]) == {1, 2, 3}
    K = 4 * lanes
    assert set(tab.npk[tab.sub == "kpass"]) == {K - 1, K, K + 1}
    assert set(tab.npk[tab.sub == "end_eq"]) == {1, 5, 100, K - 1, K, K + 3}          # packet k itself is not sent
    young = tab.sub == "young"
    assert (young & (counts[:, sc.REFUSED_TIME] > 0)).sum() >= FLOOR // 2 and (young & (counts[:, sc.REFUSED_QUEUE] > 0)).sum() >= FLOOR // 2


@pytest.mark.parametrize("lanes", LANES)
def test_queue_edges_end_their_passes(lanes):
    tab = sc.queue_edges(lanes)
    counts, _ = tab.mirror()
    closed = counts[:, sc.PASS_A] + counts[:, sc.PASS_BSCAN] + counts[:, sc.PASS_BFREE] + counts[:, sc.PASS_C]
    for sub in ("grow_above", "grow_inside", "grow_pow2", "drain", "x0zero", "gapeq"):
        assert n_where(tab, counts, sub, closed > 0) >= FLOOR, sub
    # a pass that a packet ended (the queue crossed the power of two / ran empty) is followed by another pass: more than one
    assert n_where(tab, counts, "grow_above", closed + counts[:, sc.PASS_CHAIN] + counts[:, sc.PASS_S] >= 2) >= FLOOR
    if lanes == 64:
        assert n_where(tab, counts, "drain", (counts[:, sc.PASS_BFREE] > 0) & (counts[:, sc.PASS_A] > 0)) >= FLOOR    # backlogged, then empty
    else:
        # (a queue that regime B can follow down to empty lives in the binade of 1/bw, where the 1 024 positions of a team pass do not
        # fit an int64 in units of ulp(q): the team refuses, the chain drains the queue, regime A takes over)
        assert n_where(tab, counts, "drain", (counts[:, sc.REFUSED_QUEUE] > 0) & (counts[:, sc.PASS_A] > 0)) >= FLOOR
    assert n_where(tab, counts, "x0zero", counts[:, sc.PASS_A] > 0) >= FLOOR // 3


@pytest.mark.parametrize("lanes", LANES)
def test_free_mode_on_each_side_of_the_margin(lanes):
    tab = sc.free_margin(lanes)
    counts, _ = tab.mirror()
    assert n_where(tab, counts, "free", counts[:, sc.B_FREE_MODE] > 0) >= FLOOR
    assert n_where(tab, counts, "scan", (counts[:, sc.B_NOT_FREE] > 0) & (counts[:, sc.PASS_BSCAN] > 0)) >= FLOOR
    # room below kPass + 44 and the tokens running out inside the first pass: the scan is needed there
    # (no random loss in this class: the first dropped record is the first tail drop; its packet index from its send time)
    k_first = np.array([round(((tab.drp["t1"][o] - tab.drp["lat"][o]) - tab.f["t"][c]) / tab.f["gap"][c]) if tab.ref["nd"][c] else 1 << 30
                        for c, o in enumerate(tab.off[:-1])])
    in_first_pass = k_first + (tab.f["sent"] & 3) < 4 * lanes
    assert n_where(tab, counts, "scan_fast", in_first_pass & (counts[:, sc.B_FREE_MODE] == 0) & (counts[:, sc.PASS_BSCAN] > 0)) >= FLOOR


@pytest.mark.parametrize("lanes", LANES)
def test_token_shortage_starts_at_every_listed_lane(lanes):
    tab = sc.token_patterns(lanes)
    counts, _ = tab.mirror()
    first = counts[:, sc.FIRST_SHORT] - 1
    edge = tab.sub == "edge"
    for l in sc.edge_lanes_of(lanes):
        assert (edge & (first // 4 == l)).sum() >= FLOOR, l
        for i in range(4):
            assert (edge & (first == 4 * l + i)).sum() >= 10, (l, i)
    for sub in ("none", "all", "alt"):
        assert (tab.sub == sub).sum() >= FLOOR
    assert (tab.ref["na"][tab.sub == "all"] == 0).all()
    assert n_where(tab, counts, "none", counts[:, sc.PASS_BSCAN] > 0) >= FLOOR


@pytest.mark.parametrize("lanes", LANES)
def test_philox_alignment_and_wrap_and_overrun(lanes):
    tab = sc.philox_alignment(lanes)
    for sent in range(4):
        for lr in (0.0, 1.0, 0.3):
            assert (((tab.f["sent"] & 3) == sent) & (tab.f["lr"] == lr)).sum() >= 10
    assert (tab.cases["always"][tab.f["lr"] == 1.0] == 1).all() and (tab.cases["thr"][tab.f["lr"] == 0.0] == 0).all()
    for trace in (0, 1):
        w = sc.ring_wrap(lanes, trace)
        na, nd, a0, d0 = w.ref["na"].astype(np.int64), w.ref["nd"].astype(np.int64), w.f["a"].astype(np.int64), w.f["d"].astype(np.int64)
        assert set(w.cap) == {64, 128, 256, 512}
        # no two records of one pass share a slot: a ring smaller than a pass holds its whole interval
        small = w.cap < 4 * lanes
        assert (na[small] <= w.cap[small]).all() and (nd[small] <= 2 * w.cap[small]).all()
        if lanes == 64:
            assert ((na > w.cap) & ~small).sum() >= FLOOR and ((nd > 2 * w.cap) & ~small).sum() >= FLOOR     # ... a larger one is overrun, pass after pass
        # the accepted and the dropped run both cross the ring's end, and between them the start cursors meet every lane residue
        assert ((a0 % w.cap) + na > w.cap).sum() >= FLOOR
        assert ((d0 % (2 * w.cap)) + nd > 2 * w.cap).sum() >= FLOOR
        assert len(set((a0 % 64).tolist())) == 64 and len(set((d0 % 64).tolist())) == 64
        if not trace:
            assert (a0 + na >= (1 << 32)).sum() >= FLOOR and (d0 + nd >= (1 << 32)).sum() >= FLOOR       # the cursors themselves wrap
    j = sc.trace_overrun(lanes)
    flagged = j.want["flags"] == sc.FLAG_TRACE_OVERRUN
    for sub, want in (("closed", True), ("exact", False), ("one_short", True), ("one_more", False), ("empty", True), ("serial", True),
                      ("serial_exact", False), ("serial_short", True)):
        assert (flagged[j.sub == sub] == want).all(), sub


def test_two_sender_classes_take_their_passes():
    for trace in (0, 1):
        tab = sc.pairs(trace)
        counts, _ = tab.mirror()
        f = tab.f
        assert ((tab.sub == "equal") & (f["t"][:, 0] == f["t"][:, 1]) & (f["gap"][:, 0] == f["gap"][:, 1])).sum() >= FLOOR
        r = f["gap"].max(axis=1) / f["gap"].min(axis=1)
        assert ((tab.sub == "ratio25") & (r == 25.0)).sum() >= FLOOR
        assert ((tab.sub == "beyond") & ((tab.ref["a"] + tab.ref["d"]).min(axis=1) == 0)).sum() >= FLOOR
        assert ((tab.sub == "caps") & (tab.cap[:, 0] != tab.cap[:, 1])).sum() >= FLOOR
        # class h for two senders: every alignment of the merged stream's Philox blocks with every kind of loss rate
        align = f["sent"].astype(np.int64).sum(axis=1) & 3
        for v in range(4):
            assert (align == v).sum() >= FLOOR
            for lr in (0.0, 1.0, 0.3):
                assert ((align == v) & (f["lr"] == lr) & np.char.startswith(tab.sub, "h_lr")).sum() >= 12, (v, lr)
        always = f["lr"] == 1.0
        assert always.sum() >= FLOOR and (tab.cases["always"][always] == 1).all() and (tab.cases["thr"][f["lr"] == 0.0] == 0).all()
        # ... with lr = 1 every packet is dropped, both senders send, and the link is never touched
        assert (tab.ref["a"][always] == 0).all() and (tab.ref["d"][always].min(axis=1) > 0).all()
        assert (tab.ref["q"][always].view(np.int64) == f["q"][always].view(np.int64)).all()
        assert (tab.ref["tu"][always].view(np.int64) == f["tu"][always].view(np.int64)).all()
        assert (always & (counts[:, 1] > 0)).sum() >= 12 and (always & (counts[:, 3] > 0)).sum() >= 12 and (always & (counts[:, 7] > 0)).sum() >= 12
        assert (counts[:, 1] > 0).sum() >= FLOOR and (counts[:, 3] > 0).sum() >= FLOOR     # token passes and sweeps
        # the token pass's tie: it starts the interval on an all-even state, and leaves an odd one to the sweeps
        assert ((tab.sub == "tie_even") & (counts[:, 0] > 0)).sum() >= FLOOR
        assert ((tab.sub == "tie_odd") & (counts[:, 2] > 0)).sum() >= FLOOR
    empty, _ = sc.fuzz2(2, 1).mirror()
    busy, _ = sc.fuzz2(3, 0).mirror()
    assert (empty[:, 3] + empty[:, 5] > 0).sum() >= FLOOR and (busy[:, 3] + busy[:, 5] > 0).sum() >= FLOOR
