"""Case tables and references for the wave passes of the send half (pcc-rl_amd/csrc/pcc_wave_pass.h: heavy_mi, heavy_mi2) as
tests/kernels/send_pass_harness.hip runs them, one monitor interval per case.  TEST INFRASTRUCTURE.

The reference is the plain per-packet recurrence and nothing else: `serial_mi` of send_pass_model.c for one sender, `plain` of
send_pass2_model.c (the merged recurrence) for two, through the entries pcc_cases_plain / pcc_cases2_plain.  The CPU mirrors of the
passes (`model_mi`; the token and sweep passes of the two-sender model) run on the same cases through pcc_cases_mirror /
pcc_cases2_mirror and say, per case, which regime carried how many packets and why a pass was refused: that is what
tests/test_send_pass_cases_cpu.py proves the coverage of the tables with, and what the device's own counters are held to.

A table is built for a pass length: 64 lanes (kPass = 256: a wavefront) or 256 lanes (kPass = 1 024: a team of four).
Classes (`name` of a table; `sub` labels the cases inside it):
  a / b   the plain fuzz / the straddle fuzz (regime C) of send_pass_model.c, durations cut to the packet limit; TRACE and Philox
  c       rounding ties of 1/bw: 1/bw = (2k+1) 2^-54 with q in [0.5, 1) -- all-even states (the pass runs), odd ones (it refuses)
          -- and the analogue for regime C's fabs(errv) == 0.5 v
  d       send-time edges: the top of t's binade cutting a pass at every lane position and wavefront, `end` on a send time, inside
          lane 0's block, at or before t, one packet, kPass - 1 / kPass / kPass + 1 packets, young clocks
  e       queue edges: growing through a power of two, draining to empty, x0 == 0, gap == 1/bw
  f       the free-mode margin, room of kPass + 42 .. kPass + 46 packets
  g       token patterns under TRACE: no loss, all lost, alternating, the first tail drop on every position of the row-edge lanes
          of lind_exclusive_scan (and of the wavefront edges of a team)
  h       Philox block alignment: sent & 3 = 0..3 with lr = 0, lr = 1 and a middling lr
  i       ring wrap: caps 64..512, cursors at every lane residue, cursors wrapping 2^32
  j       trace overrun: the stride ending inside a closed-form pass, inside a serial pass, exactly at the last packet
  k*      two senders: fuzz, equal send times, gaps 25 : 1, one sender beyond `end`, different caps, runs-empty and busy-period
          generators, the token pass's rounding ties, and class h for two senders: every (sent0 + sent1) & 3 with lr = 0, lr = 1
          (`always`: nothing reaches the queue) and a middling lr
"""
import ctypes
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

KEY0, KEY1 = 0x2545F491, 0x9E3779B1      # the launch's Philox key
MAX_PACKETS = 4096                       # per sender and interval (the harness's packet cap of a wavefront launch)
TEAM_MAX_PACKETS = 5 * 1024              # ... of a team launch
FLAG_TRACE_OVERRUN = 2
MIRROR_COLS, MIRROR2_COLS = 24, 8
# columns of the one-sender mirror's counts (pcc_cases_mirror)
(PASS_A, PK_A, PASS_BSCAN, PK_BSCAN, PASS_BFREE, PK_BFREE, PASS_C, PK_C, PASS_S, PK_S, PASS_CHAIN, PK_CHAIN, TIE_RUN, TIE_REFUSED,
 TOP_CUT, B_FREE_MODE, B_NOT_FREE, FIRST_SHORT, C_TIE_REFUSED, REFUSED_TIME, REFUSED_QUEUE, NOTHING, HELD, TOP_POS) = range(24)

CASE1 = np.dtype([("q", "f8"), ("tu", "f8"), ("t", "f8"), ("dl", "f8"), ("lr", "f8"), ("maxq", "f8"), ("ebw", "f8"), ("gap", "f8"),
                  ("end", "f8"), ("a", "u4"), ("d", "u4"), ("sent", "u4"), ("thr", "u4"), ("always", "u4"), ("episode", "u4"),
                  ("mi", "u4"), ("gid", "u4"), ("cap", "u4"), ("pad", "u4"), ("ring_off", "u8"), ("trace_off", "i8"),
                  ("trace_stride", "i8")])
OUT1 = np.dtype([("q", "i8"), ("tu", "i8"), ("t", "i8"), ("a", "u4"), ("d", "u4"), ("sent", "u4"), ("flags", "u4")])
CASE2 = np.dtype([("q", "f8"), ("tu", "f8"), ("t", "f8", 2), ("dl", "f8"), ("lr", "f8"), ("maxq", "f8"), ("ebw", "f8"), ("gap", "f8", 2),
                  ("end", "f8"), ("a", "u4", 2), ("d", "u4", 2), ("sent", "u4", 2), ("thr", "u4"), ("always", "u4"), ("episode", "u4"),
                  ("mi", "u4"), ("gid", "u4"), ("pad", "u4"), ("cap", "u4", 2), ("ring_off", "u8", 2), ("trace_off", "i8"),
                  ("trace_stride", "i8")])
OUT2 = np.dtype([("q", "i8"), ("tu", "i8"), ("t", "i8", 2), ("a", "u4", 2), ("d", "u4", 2), ("sent", "u4", 2), ("flags", "u4"), ("pad", "u4")])
assert CASE1.itemsize == 136 and OUT1.itemsize == 40 and CASE2.itemsize == 176 and OUT2.itemsize == 64
# the models' own layouts
MCASE1 = np.dtype([("q", "f8"), ("tu", "f8"), ("t", "f8"), ("dl", "f8"), ("lr", "f8"), ("maxq", "f8"), ("ebw", "f8"), ("gap", "f8"),
                   ("end", "f8"), ("sent", "u4"), ("pad", "u4")])
MOUT1 = np.dtype([("q", "f8"), ("tu", "f8"), ("t", "f8"), ("sent", "u4"), ("na", "u4"), ("nd", "u4"), ("pad", "u4")])
MCASE2 = np.dtype([("q", "f8"), ("tu", "f8"), ("t", "f8", 2), ("dl", "f8"), ("lr", "f8"), ("maxq", "f8"), ("ebw", "f8"), ("gap", "f8", 2),
                   ("end", "f8"), ("sent", "u4", 2)])
MOUT2 = np.dtype([("q", "f8"), ("tu", "f8"), ("t", "f8", 2), ("a", "u4", 2), ("d", "u4", 2)])
assert MCASE1.itemsize == 80 and MOUT1.itemsize == 40 and MCASE2.itemsize == 96 and MOUT2.itemsize == 48
REC = np.dtype([("t1", "f8"), ("lat", "f8")])

P = ctypes.c_void_p


def _ptr(a):
    return a.ctypes.data_as(P)


def _compile(src, lib, extra=()):
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off"] + list(extra) + [src, "-o", lib, "-lm"])
    return ctypes.CDLL(lib)


@functools.lru_cache(maxsize=None)
def model1():
    """send_pass_model.c (built as tests/test_send_pass_model.py builds it)"""
    L = _compile(os.path.join(HERE, "send_pass_model.c"), os.path.join(HERE, "libsend_pass_model.so"), ["-fopenmp"])
    L.pcc_cases_fuzz.restype = ctypes.c_long
    L.pcc_cases_fuzz.argtypes = [ctypes.c_long, ctypes.c_uint64, ctypes.c_int, ctypes.c_double, P]
    L.pcc_cases_plain.restype = ctypes.c_long
    L.pcc_cases_plain.argtypes = [ctypes.c_long, P, P, P, P, P, P]
    L.pcc_cases_mirror.restype = ctypes.c_long
    L.pcc_cases_mirror.argtypes = [ctypes.c_long, P, P, P, ctypes.c_int, P, P, P, P]
    L.pcc_cases_philox_loss.restype = None
    L.pcc_cases_philox_loss.argtypes = [ctypes.c_long] + [ctypes.c_uint32] * 7 + [ctypes.c_int, P]
    return L


@functools.lru_cache(maxsize=None)
def model2():
    L = _compile(os.path.join(HERE, "send_pass2_model.c"), os.path.join(HERE, "libsend_pass2_model.so"))
    L.pcc_cases2_fuzz.restype = ctypes.c_long
    L.pcc_cases2_fuzz.argtypes = [ctypes.c_long, ctypes.c_uint64, ctypes.c_int, ctypes.c_double, P, P]
    L.pcc_cases2_plain.restype = ctypes.c_long
    L.pcc_cases2_plain.argtypes = [ctypes.c_long] + [P] * 8
    L.pcc_cases2_mirror.restype = ctypes.c_long
    L.pcc_cases2_mirror.argtypes = [ctypes.c_long] + [P] * 9
    return L


def thr_of(lr):
    """(thr, always) as the send half derives them from the loss rate: u32_to_unit(x) < lr  <=>  x < ceil(lr 2^32)"""
    thr_d = float(np.ceil(lr * 4294967296.0))
    always = thr_d >= 4294967296.0
    return (0xFFFFFFFF if always else (int(thr_d) if thr_d > 0.0 else 0)), int(always)


def philox_loss(n, sent0, mi, episode, gid, lr):
    out = np.zeros(max(n, 1), dtype=np.uint8)
    thr, always = thr_of(lr)
    model1().pcc_cases_philox_loss(n, sent0 & 0xFFFFFFFF, mi, episode, gid, KEY0, KEY1, thr, always, _ptr(out))
    return out[:n]


def pow2ceil(x):
    p = 1
    while p < x:
        p *= 2
    return p


def packets_bound(t, gap, end):
    """room for the packets of one sender's interval (the models check it)"""
    return (int((end - t) / gap) + 6) if end > t else 2


def valid_clock(t, gap, end, max_packets):
    """the harness's clock_ok, restated"""
    if not (np.isfinite(t) and np.isfinite(gap) and np.isfinite(end) and gap > 0.0 and t >= 0.0):
        return False
    if not (t + gap > t) or not (abs(end) + gap > abs(end)):
        return False
    return (not end > t) or (end - t) / gap <= float(max_packets)


def valid_ring(arena_records, off, cap):
    """the harness's ring_ok, restated"""
    return 64 <= cap <= (1 << 20) and (cap & (cap - 1)) == 0 and off <= arena_records and 3 * cap <= arena_records - off


GUARD = 64   # untouched records between two rings: a store just past a ring lands on prefill, not on a neighbour


class Table1:
    """One sender.  f: the per-case fields (q, tu, t, dl, lr, maxq, ebw, gap, end as float64; sent, a, d, episode, mi, gid as
    uint32).  trace: the loss decisions come from `uniforms` (one array per case: uniform k belongs to the case's k-th packet;
    a case sees the first n_vis of them -- its trace stride ends there) instead of Philox.  caps: ring capacities, or None for
    rings sized to hold every record."""

    def __init__(self, name, lanes, trace, f, sub, uniforms=None, n_vis=None, caps=None):
        self.name, self.lanes, self.trace, self.f, self.sub = name, lanes, trace, f, np.array(sub)
        self.n = len(self.sub)
        self.uniforms, self.n_vis, self.caps = uniforms, n_vis, caps
        self.max_packets = MAX_PACKETS if lanes == 64 else TEAM_MAX_PACKETS
        self._done = False

    def select(self, idx):
        idx = np.asarray(idx)
        f = {k: v[idx] for k, v in self.f.items()}
        return Table1(self.name, self.lanes, self.trace, f, self.sub[idx], None if self.uniforms is None else [self.uniforms[i] for i in idx],
                      None if self.n_vis is None else [self.n_vis[i] for i in idx], None if self.caps is None else [self.caps[i] for i in idx])

    # ---- the reference
    def finish(self):
        if self._done:
            return self
        f, n = self.f, self.n
        bound = np.array([packets_bound(f["t"][c], f["gap"][c], f["end"][c]) for c in range(n)], dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(bound)]).astype(np.int64)
        total = int(self.off[-1])
        self.loss = np.zeros(total + 8, dtype=np.uint8)
        self.vis = np.zeros(n, dtype=np.int64)
        for c in range(n):
            o, b = int(self.off[c]), int(bound[c])
            if self.trace:
                u = np.asarray(self.uniforms[c], dtype=np.float64)
                nv = len(u) if self.n_vis is None or self.n_vis[c] is None else int(self.n_vis[c])
                self.vis[c] = nv
                m = min(nv, b, len(u))
                self.loss[o:o + m] = u[:m] < f["lr"][c]     # (beyond the stride: not lost)
            else:
                self.loss[o:o + b] = philox_loss(b, int(f["sent"][c]), int(f["mi"][c]), int(f["episode"][c]), int(f["gid"][c]), float(f["lr"][c]))
        self.mcase = np.zeros(n, dtype=MCASE1)
        for k in ("q", "tu", "t", "dl", "lr", "maxq", "ebw", "gap", "end", "sent"):
            self.mcase[k] = f[k]
        self.ref = np.zeros(n, dtype=MOUT1)
        self.acc = np.zeros(total + 8, dtype=REC)
        self.drp = np.zeros(total + 8, dtype=REC)
        rc = model1().pcc_cases_plain(n, _ptr(self.mcase), _ptr(self.loss), _ptr(self.off), _ptr(self.ref), _ptr(self.acc), _ptr(self.drp))
        assert rc == 0, "%s: case %d does not fit its room" % (self.name, -rc - 1)
        self.npk = self.ref["na"].astype(np.int64) + self.ref["nd"]
        # ---- rings, arena, trace
        na, nd = self.ref["na"].astype(np.int64), self.ref["nd"].astype(np.int64)
        if self.caps is None:
            self.cap = np.array([max(64, pow2ceil(max(int(na[c]), (int(nd[c]) + 1) // 2))) for c in range(n)], dtype=np.int64)
        else:
            self.cap = np.array(self.caps, dtype=np.int64)
        self.ring_off = GUARD + np.concatenate([[0], np.cumsum(3 * self.cap + GUARD)[:-1]]).astype(np.int64)
        self.arena_records = int(self.ring_off[-1] + 3 * self.cap[-1] + GUARD) if n else GUARD
        p0 = f["a"].astype(np.int64) + f["d"].astype(np.int64)
        if self.trace:
            assert int(p0.max()) < (1 << 20), "TRACE cases keep their cursors small: the row starts at position 0"
            rows, toff, o = [], np.zeros(n, dtype=np.int64), 0
            for c in range(n):
                u = np.asarray(self.uniforms[c], dtype=np.float64)[:int(self.vis[c])]
                assert len(u) == self.vis[c]
                rows.append(np.concatenate([np.zeros(int(p0[c])), u]))   # (positions before the case: 0.0 = "lost" if anybody read them)
                toff[c] = o
                o += len(rows[-1])
            self.trace_arr = np.concatenate(rows + [np.zeros(1)])
            self.trace_off, self.trace_stride = toff, p0 + self.vis
        else:
            self.trace_arr, self.trace_off, self.trace_stride = None, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        cs = np.zeros(n, dtype=CASE1)
        for k in ("q", "tu", "t", "dl", "lr", "maxq", "ebw", "gap", "end", "a", "d", "sent", "episode", "mi", "gid"):
            cs[k] = f[k]
        ta = [thr_of(float(x)) for x in f["lr"]]
        cs["thr"], cs["always"] = [x[0] for x in ta], [x[1] for x in ta]
        cs["cap"], cs["ring_off"], cs["trace_off"], cs["trace_stride"] = self.cap, self.ring_off, self.trace_off, self.trace_stride
        self.cases = cs
        # ---- what the device must leave behind
        want = np.zeros(n, dtype=OUT1)
        want["q"], want["tu"], want["t"] = self.ref["q"].view(np.int64), self.ref["tu"].view(np.int64), self.ref["t"].view(np.int64)
        want["a"] = (f["a"].astype(np.int64) + na) & 0xFFFFFFFF
        want["d"] = (f["d"].astype(np.int64) + nd) & 0xFFFFFFFF
        want["sent"] = (f["sent"].astype(np.int64) + self.npk) & 0xFFFFFFFF
        want["flags"] = np.where(self.trace & (p0 + self.npk > self.trace_stride), FLAG_TRACE_OVERRUN, 0) if self.trace else 0
        self.want = want
        self._done = True
        return self

    def prefill(self):
        return np.full((self.arena_records, 2), np.nan, dtype=np.float64)

    def want_arena(self):
        """the arena after the launch: prefill, and in every ring slot the LAST record the reference sends there"""
        ar = self.prefill()
        for c in range(self.n):
            _place(ar, int(self.ring_off[c]), int(self.cap[c]), int(self.f["a"][c]), int(self.f["d"][c]),
                   self.acc[int(self.off[c]):int(self.off[c]) + int(self.ref["na"][c])], self.drp[int(self.off[c]):int(self.off[c]) + int(self.ref["nd"][c])])
        return ar

    def mirror(self):
        """(counts [n, MIRROR_COLS], the mirror equals the plain recurrence bit for bit)"""
        self.finish()
        out, acc, drp = np.zeros(self.n, dtype=MOUT1), np.zeros_like(self.acc), np.zeros_like(self.drp)
        counts = np.zeros((self.n, MIRROR_COLS), dtype=np.uint64)
        rc = model1().pcc_cases_mirror(self.n, _ptr(self.mcase), _ptr(self.loss), _ptr(self.off), self.lanes, _ptr(out), _ptr(acc), _ptr(drp), _ptr(counts))
        assert rc == 0, (self.name, rc)
        same = out.tobytes() == self.ref.tobytes() and acc.tobytes() == self.acc.tobytes() and drp.tobytes() == self.drp.tobytes()
        return counts.astype(np.int64), same


def _place(ar, ring_off, cap, a0, d0, acc, drp):
    for recs, base, start, size in ((acc, ring_off, a0, cap), (drp, ring_off + cap, d0, 2 * cap)):
        m = len(recs)
        if not m:
            continue
        lo = max(0, m - size)     # (earlier records are overwritten)
        slots = (start + np.arange(lo, m, dtype=np.int64)) & (size - 1)
        ar[base + slots, 0] = recs["t1"][lo:]
        ar[base + slots, 1] = recs["lat"][lo:]


class Table2:
    """Two senders on one link: t, gap, sent, a, d are [n, 2]; caps None or [n, 2]."""

    def __init__(self, name, trace, f, sub, uniforms=None, caps=None):
        self.name, self.trace, self.f, self.sub = name, trace, f, np.array(sub)
        self.n, self.uniforms, self.caps = len(self.sub), uniforms, caps
        self.max_packets = MAX_PACKETS
        self._done = False

    def finish(self):
        if self._done:
            return self
        f, n = self.f, self.n
        bound = np.array([packets_bound(f["t"][c, 0], f["gap"][c, 0], f["end"][c]) + packets_bound(f["t"][c, 1], f["gap"][c, 1], f["end"][c])
                          for c in range(n)], dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(bound)]).astype(np.int64)
        total = int(self.off[-1])
        self.loss = np.zeros(total + 8, dtype=np.uint8)
        self.vis = np.zeros(n, dtype=np.int64)
        sent_all = f["sent"].astype(np.int64).sum(axis=1)
        for c in range(n):
            o, b = int(self.off[c]), int(bound[c])
            if self.trace:
                u = np.asarray(self.uniforms[c], dtype=np.float64)
                self.vis[c] = len(u)
                m = min(len(u), b)
                self.loss[o:o + m] = u[:m] < f["lr"][c]
            else:
                self.loss[o:o + b] = philox_loss(b, int(sent_all[c]), int(f["mi"][c]), int(f["episode"][c]), int(f["gid"][c]), float(f["lr"][c]))
        self.mcase = np.zeros(n, dtype=MCASE2)
        for k in ("q", "tu", "t", "dl", "lr", "maxq", "ebw", "gap", "end", "sent"):
            self.mcase[k] = f[k]
        self.ref = np.zeros(n, dtype=MOUT2)
        self.recs = [np.zeros(total + 8, dtype=REC) for _ in range(4)]     # acc0, drp0, acc1, drp1
        rc = model2().pcc_cases2_plain(n, _ptr(self.mcase), _ptr(self.loss), _ptr(self.off), _ptr(self.ref), *[_ptr(r) for r in self.recs])
        assert rc == 0, "%s: case %d does not fit its room" % (self.name, -rc - 1)
        na, nd = self.ref["a"].astype(np.int64), self.ref["d"].astype(np.int64)
        self.npk = (na + nd).sum(axis=1)
        if self.caps is None:
            self.cap = np.array([[max(64, pow2ceil(max(int(na[c, s]), (int(nd[c, s]) + 1) // 2))) for s in range(2)] for c in range(n)], dtype=np.int64)
        else:
            self.cap = np.array(self.caps, dtype=np.int64)
        sizes = (3 * self.cap + GUARD).reshape(-1)
        self.ring_off = (GUARD + np.concatenate([[0], np.cumsum(sizes)[:-1]])).astype(np.int64).reshape(n, 2)
        self.arena_records = int(self.ring_off[-1, 1] + 3 * self.cap[-1, 1] + GUARD)
        p0 = f["a"].astype(np.int64).sum(axis=1) + f["d"].astype(np.int64).sum(axis=1)
        if self.trace:
            rows, toff, o = [], np.zeros(n, dtype=np.int64), 0
            for c in range(n):
                rows.append(np.concatenate([np.zeros(int(p0[c])), np.asarray(self.uniforms[c], dtype=np.float64)]))
                toff[c] = o
                o += len(rows[-1])
            self.trace_arr = np.concatenate(rows + [np.zeros(1)])
            self.trace_off, self.trace_stride = toff, p0 + self.vis
        else:
            self.trace_arr, self.trace_off, self.trace_stride = None, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        cs = np.zeros(n, dtype=CASE2)
        for k in ("q", "tu", "t", "dl", "lr", "maxq", "ebw", "gap", "end", "a", "d", "sent", "episode", "mi", "gid"):
            cs[k] = f[k]
        ta = [thr_of(float(x)) for x in f["lr"]]
        cs["thr"], cs["always"] = [x[0] for x in ta], [x[1] for x in ta]
        cs["cap"], cs["ring_off"], cs["trace_off"], cs["trace_stride"] = self.cap, self.ring_off, self.trace_off, self.trace_stride
        self.cases = cs
        want = np.zeros(n, dtype=OUT2)
        want["q"], want["tu"], want["t"] = self.ref["q"].view(np.int64), self.ref["tu"].view(np.int64), self.ref["t"].view(np.int64)
        want["a"] = (f["a"].astype(np.int64) + na) & 0xFFFFFFFF
        want["d"] = (f["d"].astype(np.int64) + nd) & 0xFFFFFFFF
        want["sent"] = (f["sent"].astype(np.int64) + na + nd) & 0xFFFFFFFF
        want["flags"] = np.where(p0 + self.npk > self.trace_stride, FLAG_TRACE_OVERRUN, 0) if self.trace else 0
        self.want = want
        self._done = True
        return self

    def prefill(self):
        return np.full((self.arena_records, 2), np.nan, dtype=np.float64)

    def want_arena(self):
        ar = self.prefill()
        for c in range(self.n):
            o = int(self.off[c])
            for s in range(2):
                _place(ar, int(self.ring_off[c, s]), int(self.cap[c, s]), int(self.f["a"][c, s]), int(self.f["d"][c, s]),
                       self.recs[2 * s][o:o + int(self.ref["a"][c, s])], self.recs[2 * s + 1][o:o + int(self.ref["d"][c, s])])
        return ar

    def mirror(self):
        self.finish()
        out = np.zeros(self.n, dtype=MOUT2)
        recs = [np.zeros_like(r) for r in self.recs]
        counts = np.zeros((self.n, MIRROR2_COLS), dtype=np.uint64)
        rc = model2().pcc_cases2_mirror(self.n, _ptr(self.mcase), _ptr(self.loss), _ptr(self.off), _ptr(out), *[_ptr(r) for r in recs], _ptr(counts))
        assert rc == 0, (self.name, rc)
        same = out.tobytes() == self.ref.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(recs, self.recs))
        return counts.astype(np.int64), same


# ================================================================================================ builders, one sender
class _Rows:
    """collects cases one by one"""
    FLOATS = ("q", "tu", "t", "dl", "lr", "maxq", "ebw", "gap", "end")
    INTS = ("sent", "a", "d", "episode", "mi", "gid")

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.rows, self.sub, self.uniforms, self.n_vis, self.caps = [], [], [], [], []

    def add(self, sub, q, tu, t, maxq, ebw, gap, end, dl=None, lr=0.0, sent=0, a=None, d=None, u=None, n_vis=None, cap=None):
        r = self.rng
        self.rows.append(dict(q=q, tu=tu, t=t, dl=0.05 + 0.4 * r.random() if dl is None else dl, lr=lr, maxq=maxq, ebw=ebw, gap=gap, end=end,
                              sent=sent, a=int(r.integers(0, 300)) if a is None else a, d=int(r.integers(0, 300)) if d is None else d,
                              episode=int(r.integers(0, 1 << 16)), mi=int(r.integers(0, 400)), gid=int(r.integers(0, 1 << 20))))
        self.sub.append(sub)
        self.uniforms.append(u)
        self.n_vis.append(n_vis)
        self.caps.append(cap)

    def table(self, name, lanes, trace):
        f = {k: np.array([x[k] for x in self.rows], dtype=np.float64) for k in self.FLOATS}
        f.update({k: np.array([x[k] & 0xFFFFFFFF for x in self.rows], dtype=np.uint32) for k in self.INTS})
        if trace:
            # a case without uniforms of its own: a row of them for every packet it can send (and the passes' look-ahead)
            for c, x in enumerate(self.rows):
                if self.uniforms[c] is None:
                    self.uniforms[c] = self.rng.random(packets_bound(x["t"], x["gap"], x["end"]) + 4 * lanes + 8)
                    if self.n_vis[c] is None:
                        self.n_vis[c] = len(self.uniforms[c])
        caps = None if all(c is None for c in self.caps) else self.caps
        assert caps is None or all(c is not None for c in caps)
        return Table1(name, lanes, trace, f, self.sub, self.uniforms if trace else None, self.n_vis if trace else None, caps)


T0 = 100.0   # a send time deep inside [64, 128): ulp 2^-46


def _link(kind, K, i=0):
    """(q, maxq, ebw, rho) of a link state that sends by regime A ("a"), B in free mode ("free"), B with the token scan ("scan") or,
    on a wavefront, C ("c"); rho = (1/bw) / gap, the sender's rate over the link's.  i jitters the numbers."""
    j = 1.0 + 0.003 * (i % 17)
    if kind == "a":
        return 0.0, 0.5, 0.0015 * j, 0.75
    if kind == "free":
        return (1.2 * j, 7.9, 0.004 * j, 1.2) if K == 256 else (1.2 * j, 15.5, 0.004 * j, 1.2)
    if kind == "scan":
        ebw = (0.0024 if K == 256 else 0.0006) * j
        return 0.95 - 10.0 * ebw, 0.95, ebw, 1.5
    if kind == "c":
        ebw = 0.004 * j
        return 1.0 - 0.5 * ebw, 1.0 + 2.3 * ebw, ebw, 1.5
    raise ValueError(kind)


def _tu(t0, gap):
    return t0 - 0.3 * gap


@functools.lru_cache(maxsize=None)
def fuzz1(lanes, straddle, trace):
    """classes a (straddle = 0) and b (1): 1 024 cases for a wavefront; 256 for a team, where a case is a workgroup of four wavefronts
    (the same 1 024 wavefronts per launch: the size the device tests keep their largest launch to)"""
    n = 1024 if lanes == 64 else 256
    cut = (MAX_PACKETS if lanes == 64 else TEAM_MAX_PACKETS) - 8
    mc = np.zeros(n, dtype=MCASE1)
    model1().pcc_cases_fuzz(n, 1234567 + 17 * lanes + straddle, straddle, float(cut), _ptr(mc))
    rng = np.random.default_rng(99 + lanes + 2 * straddle + trace)
    f = {k: mc[k].copy() for k in _Rows.FLOATS}
    f["sent"] = mc["sent"].copy()
    f["a"], f["d"] = rng.integers(0, 500, n).astype(np.uint32), rng.integers(0, 500, n).astype(np.uint32)
    f["episode"], f["mi"], f["gid"] = (rng.integers(0, 1 << 16, n).astype(np.uint32), rng.integers(0, 400, n).astype(np.uint32),
                                       rng.integers(0, 1 << 20, n).astype(np.uint32))
    uniforms = None
    if trace:
        uniforms = [rng.random(packets_bound(f["t"][c], f["gap"][c], f["end"][c]) + 4 * lanes + 8) for c in range(n)]
    return Table1("ab"[straddle] + ("_trace" if trace else "_philox"), lanes, bool(trace), f, ["fuzz"] * n, uniforms).finish()


@functools.lru_cache(maxsize=None)
def ties(lanes):
    K, R = 4 * lanes, _Rows(301)
    u = 2.0 ** -53      # ulp of [0.5, 1)
    for i in range(64):
        ebw = float((int(0.004 * (1.0 + 0.01 * i) * 2 ** 54) | 1) * 2.0 ** -54)   # (2k+1) 2^-54: exactly half a unit of [0.5, 1)
        gap = ebw / 1.5
        q_even = float(np.round((0.9 - (5 + i % 40) * ebw) / (2 * u)) * 2 * u)
        end = T0 + (1.5 * K + i + 0.5) * gap
        R.add("even", q_even, _tu(T0, gap), T0, 0.9, ebw, gap, end, lr=0.02 * (i % 2), sent=i & 3)
        R.add("odd", q_even + u, _tu(T0, gap), T0, 0.9, ebw, gap, end, lr=0.02 * (i % 2), sent=i & 3)
        if lanes == 64:   # regime C's analogue: maxq just above B = 1, v = ulp(B) / 2 = 2^-53, 1/bw exactly half a unit of v off the grid;
            # maxq - 1/bw < B, so the full queue lands on both sides of B (below it, fl(x + 1/bw) is the tie itself)
            maxq = 1.0 + (0.3, 0.5, 0.7)[i % 3] * ebw
            q = float(np.round((maxq - 3.0 * ebw) / (2 * u)) * 2 * u) + (i & 1) * u
            R.add("ctie", q, _tu(T0, gap), T0, maxq, ebw, gap, end, sent=i & 3)
    return R.table("c", lanes, True).finish()


@functools.lru_cache(maxsize=None)
def time_edges(lanes):
    K, R = 4 * lanes, _Rows(302)
    kinds = ("a", "free", "scan")
    i = 0
    # the top of t's binade cuts the pass at position p: every lane position, every wavefront
    lanes_cut = (1, 9, 31, 63) if lanes == 64 else (1, 63, 64, 127, 128, 191, 192, 255)
    for top in (64.0, 128.0, 256.0):
        for l in lanes_cut:
            for pos in range(4):
                p = 4 * l + pos
                for kind in kinds:
                    q, maxq, ebw, rho = _link(kind, K, i)
                    gap, skip = ebw / rho, i & 3
                    kc = p - skip            # the first packet that is not below `top`
                    if kc < 3:
                        continue
                    t0 = top - (kc - 0.5) * gap
                    R.add("top", q, _tu(t0, gap), t0, maxq, ebw, gap, t0 + 1.5 * K * gap, lr=0.01 * (i % 3), sent=skip)
                    i += 1
    for kind in kinds:
        for j in range(20):
            q, maxq, ebw, rho = _link(kind, K, j)
            gap, skip = ebw / rho, j & 3
            G = (T0 + gap) - T0
            for k in (1, 5, 100, K - 1, K, K + 3)[j % 6:j % 6 + 1]:
                R.add("end_eq", q, _tu(T0, gap), T0, maxq, ebw, gap, T0 + k * G, sent=skip)     # `end` IS the send time of packet k
            R.add("lane0", q, _tu(T0, gap), T0, maxq, ebw, gap, T0 + (1 + j % 3 - 0.5) * gap, sent=skip)   # 1..3 packets
            R.add("one", q, _tu(T0, gap), T0, maxq, ebw, gap, T0 + 0.5 * gap, sent=skip)
            R.add("none", q, _tu(T0, gap), T0, maxq, ebw, gap, T0 - (j % 2) * 1.0, sent=skip)   # end == t, end < t
            for npk in (K - 1, K, K + 1):
                R.add("kpass", q, _tu(T0, gap), T0, maxq, ebw, gap, T0 + (npk - 0.5) * gap, sent=(0, 1, 3)[j % 3])
            # young clocks: t0 around (kPass + 4) gap; and tu + tu < tend
            t0 = (K + 4.0) * gap * (0.3, 0.6, 0.99, 1.0, 1.01)[j % 5]
            R.add("young", q, max(0.0, t0 - 0.3 * gap), t0, maxq, ebw, gap, t0 + 1.2 * K * gap, sent=skip)
            R.add("young", 2.0, 1.2, 3.0, 3.0, ebw, gap, 3.0 + 1.2 * K * gap, sent=skip)
    return R.table("d", lanes, True).finish()


@functools.lru_cache(maxsize=None)
def queue_edges(lanes):
    K, R = 4 * lanes, _Rows(303)
    ebw0 = 0.004 if lanes == 64 else 0.001
    for i in range(56):
        ebw = ebw0 * (1.0 + 0.002 * i)
        gap = ebw / 1.5
        grow = ebw - gap
        at = 5 + (3 if lanes == 64 else 14) * i                 # the packet that takes q across 0.5
        end = T0 + (1.5 * K + 0.5) * gap
        # growing through 0.5 with maxq above the binade: the pass ends at the crossing
        R.add("grow_above", 0.5 - at * grow, _tu(T0, gap), T0, 0.8, ebw, gap, end, lr=0.01 * (i % 2), sent=i & 3)
        # maxq inside q's binade: the queue fills up to it, just below 0.5
        R.add("grow_inside", 0.499 - at * grow, _tu(T0, gap), T0, 0.499, ebw, gap, end, sent=i & 3)
        # maxq at the power of two itself, and just above it
        R.add("grow_pow2", 0.5 - at * grow, _tu(T0, gap), T0, 0.5 + (i % 3) * 0.7 * ebw, ebw, gap, end, sent=i & 3)
        # draining to empty: the sender a little slower than the link, the queue inside the binade of 1/bw so that only "empty" ends the pass
        # (x + 1/bw stays in the binade of 1/bw all the way down to x = 0 when 1/bw sits just above a power of two)
        eb = 2.0 ** np.floor(np.log2(ebw0))
        e1 = eb * (1.01 + 0.0015 * i)
        g1 = e1 + e1 / ((16.0, 64.0, 256.0) if lanes == 64 else (64.0, 512.0, 2048.0))[i % 3]
        R.add("drain", e1 + eb * (0.2 + 0.012 * i), T0 - g1, T0, 0.5, e1, g1, T0 + (1.5 * K + 0.5) * g1, sent=i & 3)
        # x0 exactly 0: q == t0 - tu
        R.add("x0zero", 0.25, T0 - 0.25, T0, 0.9, ebw, ebw * (1.25 if i % 2 else 0.75), end, sent=i & 3)
        # gap exactly 1/bw: on the grid of t (G == 1/bw) and off it
        e_grid = float(np.round(ebw * 2.0 ** 46) * 2.0 ** -46)
        for e1 in (e_grid, ebw):
            R.add("gapeq", 0.0 if i % 2 else 0.7, _tu(T0, e1), T0, 0.9, e1, e1, T0 + (1.5 * K + 0.5) * e1, sent=i & 3)
    return R.table("e", lanes, True).finish()


def _r_of(q, ebw):
    """1/bw on the grid of ulp(q), as the pass computes it"""
    e, eb = np.floor(np.log2(q)), np.floor(np.log2(ebw))
    probe = 2.0 ** e
    return ebw if eb == e else (probe + ebw) - probe


@functools.lru_cache(maxsize=None)
def free_margin(lanes):
    K, R = 4 * lanes, _Rows(304)
    for r in (42, 43, 44, 45, 46):
        for delta in (-0.3, 0.3):
            for rho in (1.3, 2.0):
                for j in range(6):
                    ebw = 0.004 * (1.0 + 0.01 * j)
                    gap = ebw / rho
                    q = (1.1 if lanes == 64 else 4.2) + 0.01 * j
                    tu = _tu(T0, gap)
                    x0 = q - (T0 - tu)
                    Rr = _r_of(q, ebw)
                    maxq = (x0 + (K + r + delta) * Rr) + Rr
                    room = ((maxq - Rr) - x0) / Rr
                    R.add("free" if room >= K + 44.0 else "scan", q, tu, T0, maxq, ebw, gap, T0 + (K + 100.5) * gap, sent=j & 3)
    # the other side of the sign: room of kPass - 46 .. kPass - 18 packets and a sender so fast that the tokens run out INSIDE the
    # pass (a pass gets kPass / rho new tokens: the first tail drop falls at about room / (1 - 1 / rho)) -- free mode would be wrong
    for r in (-46, -44, -42, -36, -30, -24, -18):
        for rho in (32.0, 64.0, 128.0):
            for j in range(3):
                ebw = (0.004 if lanes == 64 else 0.003) * (1.0 - 0.01 * j)          # (the full queue stays inside q's binade)
                gap = ebw / rho
                q = (1.01 if lanes == 64 else 4.02) + 0.002 * j
                tu = _tu(T0, gap)
                x0 = q - (T0 - tu)
                Rr = _r_of(q, ebw)
                maxq = (x0 + (K + r + 0.5) * Rr) + Rr
                R.add("scan_fast", q, tu, T0, maxq, ebw, gap, T0 + (K + 100.5) * gap, sent=j & 3)
    return R.table("f", lanes, True).finish()


def _token_state(K, n0, rho, j=0):
    ebw = (0.0024 if K == 256 else 0.0006) * (1.0 + 0.002 * j)
    gap = ebw / rho
    tu = _tu(T0, gap)
    q = (0.95 - n0 * ebw - 0.5 * ebw) + (T0 - tu)       # room for about n0 packets in front of the first
    return q, tu, 0.95, ebw, gap


@functools.lru_cache(maxsize=None)
def token_patterns(lanes):
    """lr = 0.5 and uniforms 0.25 (lost) / 0.75 (kept): the test decides every loss"""
    K, R = 4 * lanes, _Rows(305)
    npk = K + K // 2
    keep, lost = 0.75, 0.25
    for j in range(52):
        q, tu, maxq, ebw, gap = _token_state(K, 3 + 2 * j, 1.5, j)
        end = T0 + (npk + 0.5) * gap
        R.add("none", q, tu, T0, maxq, ebw, gap, end, lr=0.5, sent=j & 3, u=np.full(npk + K + 8, keep))
        R.add("all", q, tu, T0, maxq, ebw, gap, end, lr=0.5, sent=j & 3, u=np.full(npk + K + 8, lost))
        u = np.full(npk + K + 8, keep)
        u[(j & 1)::2] = lost
        R.add("alt", q, tu, T0, maxq, ebw, gap, end, lr=0.5, sent=j & 3, u=u)
    fixed = R.table("g", lanes, True)
    # ---- the first tail drop at a chosen position: candidates over (room, rate, leading losses), picked by the mirror
    edge_lanes = edge_lanes_of(lanes)
    C = _Rows(306)
    for rho in (1.2, 1.25, 1.3, 1.4, 1.5, 1.6, 1.75, 2.0, 2.5, 3.0):
        for n0 in range(0, int(K * (1.0 - 1.0 / rho)) + 3):
            est = n0 / (1.0 - 1.0 / rho)
            if min(abs(est - 4 * l - 2) for l in edge_lanes) > 16:
                continue
            for nl in range(3):
                for skip in range(4):
                    q, tu, maxq, ebw, gap = _token_state(K, n0, rho, n0)
                    if not q - (T0 - tu) > 0.0:
                        continue
                    u = np.full(npk + K + 8, keep)
                    u[:nl] = lost                            # leading losses hold tokens back: they move the first tail drop
                    C.add("edge", q, tu, T0, maxq, ebw, gap, T0 + (npk + 0.5) * gap, lr=0.5, sent=skip, u=u)
    cand = C.table("g", lanes, True)
    counts, _ = cand.mirror()
    first = counts[:, FIRST_SHORT] - 1       # pass position of the first tail drop (-1: none)
    pick = []
    for l in edge_lanes:
        for pos in range(4):
            idx = np.flatnonzero(first == 4 * l + pos)
            pick.extend(idx[:14].tolist())
    sel = cand.select(sorted(pick))
    f = {k: np.concatenate([fixed.f[k], sel.f[k]]) for k in fixed.f}
    return Table1("g", lanes, True, f, list(fixed.sub) + list(sel.sub), fixed.uniforms + sel.uniforms, fixed.n_vis + sel.n_vis).finish()


def edge_lanes_of(lanes):
    return (0, 1, 15, 16, 17, 31, 32, 47, 48, 63) if lanes == 64 else (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255)


@functools.lru_cache(maxsize=None)
def philox_alignment(lanes):
    K, R = 4 * lanes, _Rows(307)
    kinds = ("a", "free", "scan", "c", "young")
    for kind in kinds:
        for sent in range(4):
            for lr in (0.0, 1.0, 0.3, 2.0 ** -32):
                for j in range(2):
                    q, maxq, ebw, rho = _link("scan" if kind == "young" else kind, K, j + sent)
                    gap = ebw / rho
                    t0 = (K + 4.0) * gap * 0.7 if kind == "young" else T0
                    R.add("sent%d" % sent, q, max(0.0, _tu(t0, gap)), t0, maxq, ebw, gap, t0 + (1.5 * K + 0.5) * gap, lr=lr, sent=sent + 4 * j * 5)
    return R.table("h", lanes, False).finish()


@functools.lru_cache(maxsize=None)
def ring_wrap(lanes, trace):
    """Rings of 64..512 slots whose runs of accepted and of dropped records cross the ring's end inside a pass, the start cursors at
    every lane residue (TRACE) or just below 2^32, where the cursors themselves wrap (Philox).  Which record a slot ends up with is
    defined only while no two records of ONE pass share a slot (two lanes of one store instruction, or two wavefronts of a team,
    would race for it -- the product never gets there: an interval that outgrows its rings is PCC_FLAG_RING_OVERFLOW, results
    invalid).  So a ring smaller than a pass gets an interval it can hold, about 1.2 cap packets; a ring of a pass or more gets
    seven times its capacity, and the comparison covers the last cap (dropped: 2 cap) records of the reference, slot by slot.
    A team has no overrun case at all, and not for want of a larger ring: from pass to pass a slot would be rewritten by ANOTHER
    wavefront of the workgroup, and what orders the two stores is a workgroup barrier that does not wait for vector stores to
    land -- the source does not define the winner, the product never asks for one."""
    K, R = 4 * lanes, _Rows(308 + trace)
    i = 0
    for cap in (64, 128, 256, 512):
        for r in range(64):
            q, maxq, ebw, rho = _link("scan", K, i)
            gap = ebw / rho
            if trace:       # cursors a little before the ring's end, at every lane residue
                a, d = (cap - r) % cap + cap * (i % 3), (2 * cap - 1 - r) % (2 * cap)
            else:           # ... and before 2^32, where the cursors themselves wrap
                a, d = (1 << 32) - 3 * r - 1, (1 << 32) - 5 * r - 2
            npk = 7 * cap if cap >= K else int(1.2 * cap)
            R.add("cap%d" % cap, q, _tu(T0, gap), T0, maxq, ebw, gap, T0 + (npk + 0.5) * gap, lr=0.3, sent=i & 3, a=a, d=d, cap=cap)
            i += 1
    return R.table("i_trace" if trace else "i_philox", lanes, bool(trace)).finish()


@functools.lru_cache(maxsize=None)
def trace_overrun(lanes):
    K, R = 4 * lanes, _Rows(310)
    for j in range(10):
        q, maxq, ebw, rho = _link("scan", K, j)
        gap = ebw / rho
        npk = K + 50 + j
        end = T0 + (npk - 0.5) * gap
        u = R.rng.random(npk + K + 8)
        for sub, nv in (("closed", K // 2 + j), ("exact", npk), ("one_short", npk - 1), ("one_more", npk + 1), ("empty", 0)):
            R.add(sub, q, _tu(T0, gap), T0, maxq, ebw, gap, end, lr=0.5, sent=j & 3, u=u, n_vis=nv)
        t0 = (K + 4.0) * gap * 0.5            # a young clock: serial passes
        npk2 = 40 + j
        for sub, nv in (("serial", 3 + j), ("serial_exact", npk2), ("serial_short", npk2 - 1)):
            R.add(sub, q, t0 - 0.3 * gap, t0, maxq, ebw, gap, t0 + (npk2 - 0.5) * gap, lr=0.5, sent=j & 3, u=u, n_vis=nv)
    return R.table("j", lanes, True).finish()


# the one-sender classes: name -> builder(lanes)
CLASSES1 = {
    "a_trace": lambda lanes: fuzz1(lanes, 0, 1), "a_philox": lambda lanes: fuzz1(lanes, 0, 0),
    "b_trace": lambda lanes: fuzz1(lanes, 1, 1), "b_philox": lambda lanes: fuzz1(lanes, 1, 0),
    "c": ties, "d": time_edges, "e": queue_edges, "f": free_margin, "g": token_patterns, "h": philox_alignment,
    "i_trace": lambda lanes: ring_wrap(lanes, 1), "i_philox": lambda lanes: ring_wrap(lanes, 0), "j": trace_overrun,
}


# ================================================================================================ builders, two senders
class _Rows2:
    FLOATS = ("q", "tu", "dl", "lr", "maxq", "ebw", "end")

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.rows, self.sub, self.caps = [], [], []

    def add(self, sub, q, tu, t, maxq, ebw, gap, end, lr=0.0, sent=(0, 0), a=None, d=None, cap=None):
        r = self.rng
        self.rows.append(dict(q=q, tu=tu, t=t, dl=0.05 + 0.4 * r.random(), lr=lr, maxq=maxq, ebw=ebw, gap=gap, end=end, sent=sent,
                              a=[int(x) for x in r.integers(0, 200, 2)] if a is None else a, d=[int(x) for x in r.integers(0, 200, 2)] if d is None else d,
                              episode=int(r.integers(0, 1 << 16)), mi=int(r.integers(0, 400)), gid=int(r.integers(0, 1 << 20))))
        self.sub.append(sub)
        self.caps.append(cap)

    def table(self, name, trace):
        f = {k: np.array([x[k] for x in self.rows], dtype=np.float64) for k in self.FLOATS}
        for k in ("t", "gap"):
            f[k] = np.array([x[k] for x in self.rows], dtype=np.float64).reshape(-1, 2)
        for k in ("sent", "a", "d"):
            f[k] = np.array([[v & 0xFFFFFFFF for v in x[k]] for x in self.rows], dtype=np.uint32).reshape(-1, 2)
        for k in ("episode", "mi", "gid"):
            f[k] = np.array([x[k] for x in self.rows], dtype=np.uint32)
        uniforms = None
        if trace:
            uniforms = [self.rng.random(packets_bound(x["t"][0], x["gap"][0], x["end"]) + packets_bound(x["t"][1], x["gap"][1], x["end"]) + 264)
                        for x in self.rows]
        caps = None if all(c is None for c in self.caps) else self.caps
        assert caps is None or all(c is not None for c in caps)
        return Table2(name, trace, f, self.sub, uniforms, caps)


@functools.lru_cache(maxsize=None)
def fuzz2(kind_only, trace):
    """the generators of pcc_model2_fuzz_sweeps: as drawn (kind_only = -1), only "runs empty" (2), only "busy period" (3)"""
    n = 1024 if kind_only < 0 else 256
    mc, kinds = np.zeros(n, dtype=MCASE2), np.zeros(n, dtype=np.int32)
    got = model2().pcc_cases2_fuzz(n, 424243 + kind_only, kind_only, float(MAX_PACKETS - 8), _ptr(mc), _ptr(kinds))
    assert got == n
    rng = np.random.default_rng(77 + kind_only + trace)
    R = _Rows2(500 + kind_only + trace)
    for c in range(n):
        R.add("kind%d" % kinds[c], mc["q"][c], mc["tu"][c], list(mc["t"][c]), mc["maxq"][c], mc["ebw"][c], list(mc["gap"][c]), mc["end"][c],
              lr=mc["lr"][c], sent=(int(mc["sent"][c, 0]), int(rng.integers(0, 4))))
    name = {-1: "k_fuzz", 2: "k_empty", 3: "k_busy"}[kind_only] + ("_trace" if trace else "_philox")
    return R.table(name, bool(trace)).finish()


@functools.lru_cache(maxsize=None)
def pairs(trace):
    """class k: equal send times at every position, gaps 25 : 1, one sender beyond `end`, different caps, Philox alignment, and the
    token pass's own rounding ties of 1/bw"""
    R = _Rows2(600 + trace)
    for i in range(64):
        ebw = 0.004 * (1.0 + 0.004 * i)
        lr = (0.0, 0.03, 0.3)[i % 3]
        # the same t and the same gap: every packet of sender 1 ties with one of sender 0 (sender 0 first); backlogged and near empty
        gap = ebw * (1.7 if i % 2 else 2.6)          # the pair sends at 2 / 1.7 and 2 / 2.6 of the link's rate
        q, maxq = (0.9 - (5 + i) * ebw, 0.9) if i % 2 else (0.0, 0.5)
        R.add("equal", q, _tu(T0, gap), [T0, T0], maxq, ebw, [gap, gap], T0 + (300.5 + i) * gap, lr=lr, sent=(i & 3, (i >> 2) & 3))
        # ... ties at every fourth position only: sender 1 four times as slow
        R.add("equal4", q, _tu(T0, gap), [T0, T0], maxq, ebw, [gap, 4 * gap] if i % 4 < 2 else [4 * gap, gap], T0 + (300.5 + i) * gap, lr=lr,
              sent=(i & 3, (i >> 2) & 3))
        # gaps in ratio 25 : 1
        g0 = ebw / 1.4
        R.add("ratio25", 0.9 - (5 + i) * ebw, _tu(T0, g0), [T0 + 0.3 * g0, T0], 0.9, ebw, [g0, 25 * g0] if i % 2 else [25 * g0, g0],
              T0 + (600.5 + i) * g0, lr=lr, sent=(i & 3, (i >> 2) & 3))
        # one sender's next SEND beyond `end`
        end = T0 + (400.5 + i) * g0
        R.add("beyond", 0.9 - (5 + i) * ebw, _tu(T0, g0), [T0, end + (i % 3) * g0] if i % 2 else [end + (i % 3) * g0, T0], 0.9, ebw, [g0, g0], end,
              lr=lr, sent=(i & 3, (i >> 2) & 3))
        # different caps for the two senders (a pass of 256 positions or more each: no two records of one pass share a slot), cursors
        # near the rings' ends
        c0, c1 = (256, 1024) if i % 2 else (512, 256)
        R.add("caps", 0.9 - (5 + i) * ebw, _tu(T0, g0), [T0, T0 + 0.5 * g0], 0.9, ebw, [g0, 1.5 * g0], T0 + (500.5 + i) * g0, lr=0.3,
              sent=(i & 3, (i >> 2) & 3), a=[c0 - i % c0, c1 - (3 * i) % c1], d=[2 * c0 - i, 2 * c1 - 2 * i])
    # rounding ties of 1/bw for the token pass: 1/bw = (2k+1) 2^-54 with q in [0.5, 1); all-even states (q, both send times and both
    # gaps on even multiples of ulp(q): the pass runs) and odd ones (it refuses, the sweeps take over)
    u = 2.0 ** -53
    for i in range(64):
        ebw = float((int(0.004 * (1.0 + 0.01 * i) * 2 ** 54) | 1) * 2.0 ** -54)
        gap = ebw * 1.3                              # the pair at about 1.5 times the link's rate
        q_even = float(np.round((0.9 - (5 + i % 40) * ebw) / (2 * u)) * 2 * u)
        for sub, q in (("tie_even", q_even), ("tie_odd", q_even + u)):
            R.add(sub, q, _tu(T0, gap), [T0, T0 + 0.4 * gap], 0.9, ebw, [gap, gap * 1.1], T0 + (300.5 + i) * gap, lr=0.02 * (i % 2), sent=(i & 3, (i >> 2) & 3))
    # class h for two senders: every value of (sent0 + sent1) & 3 with lr = 0 (thr = 0), lr = 1 (`always`: every packet lost at random,
    # q and tu never touched while the merge still orders the dropped records) and a middling lr; on a backlogged link (the token
    # pass), a nearly empty one (the sweeps) and a young clock (the plain recurrence)
    for v in range(4):
        for lr in (0.0, 1.0, 0.3):
            for j in range(15):
                ebw = 0.004 * (1.0 + 0.003 * (j + 4 * v))
                s0 = (j + v) & 3
                sent = (s0 + 4 * (j % 3), ((v - s0) & 3) + 4 * (j % 2))
                kind = j % 3
                if kind == 0:
                    gap, q, maxq, t0 = ebw * 1.3, 0.9 - (5 + j) * ebw, 0.9, T0
                elif kind == 1:
                    gap, q, maxq, t0 = ebw * 2.6, 0.5 * ebw, 0.5, T0
                else:
                    gap, q, maxq = ebw * 1.3, 0.9 - (5 + j) * ebw, 0.9
                    t0 = 100.0 * gap
                R.add("h_lr%g" % lr, q, max(0.0, _tu(t0, gap)), [t0, t0 + (0.0 if j % 2 else 0.4 * gap)], maxq, ebw, [gap, gap * (1.0 if j % 2 else 1.1)],
                      t0 + (300.5 + j) * gap, lr=lr, sent=sent)
    # every other case gets the caps the reference needs; "caps" gets its own -> give all of them explicit caps after the reference ran
    t = R.table("k_pairs" + ("_trace" if trace else "_philox"), bool(trace))
    caps_sub = np.array(R.sub) == "caps"
    t.finish()
    caps = t.cap.copy()
    for c in np.flatnonzero(caps_sub):
        caps[c] = (256, 1024) if (c // 5) % 2 else (512, 256)   # (the first 320 rows: five per i)
    t2 = Table2(t.name, t.trace, t.f, t.sub, t.uniforms, caps.tolist())
    return t2.finish()


CLASSES2 = {
    "k_fuzz_trace": lambda: fuzz2(-1, 1), "k_fuzz_philox": lambda: fuzz2(-1, 0), "k_empty": lambda: fuzz2(2, 1), "k_busy": lambda: fuzz2(3, 0),
    "k_pairs_trace": lambda: pairs(1), "k_pairs_philox": lambda: pairs(0),
}
