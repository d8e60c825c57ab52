"""The wave passes of the send half (pcc-rl_amd/csrc/pcc_wave_pass.h: heavy_mi as one wavefront, staged or not, and as a team of four;
heavy_mi2 staged or not; TRACE and Philox) held to the plain per-packet recurrence: the harness kernels of
tests/kernels/send_pass_harness.hip run them, unchanged, one monitor interval per case on the case tables of
tests/models/send_pass_cases.py, and the final state (q, tu, t as bits; a, d, sent; the flags) and the WHOLE arena of rings are
compared with the reference as integers or int64 views: there is no tolerance anywhere.  The arena is prefilled with NaN and the
outputs with 0xFF bytes, so a ring slot the reference never writes, the guard records between two rings and the outputs of a case
the device refused must still hold their prefill: a stray store shows.  Both builds of the harness run every table -- the plain
one and the -DPCC_PROFILE=1 one, whose passes count themselves -- and from the profile build's counters the device's closed-form
packets per regime (A, B with the scan, B without, C; the token pass and the sweeps for two senders) must be at least half of
what the CPU mirror commits by that regime on the same cases: half is the margin tests/test_path_reach.py uses (staging, the
team layout and the chain's hold-back move a pass boundary), and it rules out a class that silently fell through to the serial
pass.  What the tables cover is proved on the CPU, from the inputs and the models alone, in tests/test_send_pass_cases_cpu.py.

The harness is a separate compilation of the same source: it holds the source-level passes to the recurrence at states the
simulator rarely or never produces; it cannot vouch for the machine code of the product kernels the header is compiled into --
the simulator's parity tests hold that to the oracle.

Measured on an MI355X: the 103 tests of this file take 8 s together, tables and references included (they are built once per
session and shared); the slowest test is 0.6 s.  The largest launch is 1 024 wavefronts.  Nothing differed on the device, and one
sender's counters came out equal to the mirror's packet for packet.

With PCC_SEND_PASS_REPORT=<file> in the environment the device's and the mirror's counts per table are written there as JSON
(profiles/r27_send_pass_cases.json was made that way)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import pcc_rl_amd   # noqa: F401
from pcc_rl_amd import build as pbuild

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import send_pass_cases as sc   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, I64, I32, U32, U64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
VARIANTS = {"wave": (0, 64), "staged": (1, 64), "team": (2, 256)}     # entry -> (variant of pcc_test_send1, lanes of a pass)
# what pcc_test_send_packet_slot(which) names: the harness answers with the slot of a stats block, from the PCC_PATH_* enum it was built with
WHICH1 = {"A": 0, "B_scan": 1, "B_free": 2, "C": 3, "serial": 4}
WHICH_TEAM = {"A": 5, "B_scan": 6, "B_free": 7, "C": 8, "serial": 9}
WHICH2 = {"token": 10, "sweep256": 11, "sweep64": 12, "plain": 13}
MIRROR_COLS1 = {"A": sc.PK_A, "B_scan": sc.PK_BSCAN, "B_free": sc.PK_BFREE, "C": sc.PK_C}
REPORT = {}


@pytest.fixture(scope="module")
def harness():
    libs = {}
    for build, path in zip(("plain", "profile"), pbuild.build_send_harness()):   # (a tree built the usual way has both: this compiles only what is missing or stale)
        L = ctypes.CDLL(path)
        for f in (L.pcc_test_send1, L.pcc_test_send2):
            f.restype = I32
            f.argtypes = [I32, I32, P, I64, P, U64, P, I64, U32, U32, U32, P, P, P]
        libs[build] = L
    assert libs["plain"].pcc_test_send_profile() == 0 and libs["profile"].pcc_test_send_profile() == 1
    yield libs
    # the counts of the profile-build tests of this session, for profiles/
    path = os.environ.get("PCC_SEND_PASS_REPORT")
    if path and REPORT:
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        old["tables"] = {k: REPORT[k] for k in sorted(REPORT)}
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def counted(L, stats, which):
    """packets per path of a stats block, the slots asked of the harness"""
    out = {}
    for k, w in which.items():
        slot = L.pcc_test_send_packet_slot(w)
        assert 16 <= slot < len(stats), (k, slot)
        out[k] = int(stats[slot])
    return out


def to_dev(a):
    return torch.as_tensor(np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8).copy(), device=DEV)


def launch(L, fn, variant, tab, profile):
    """-> (outputs as a structured array, the arena as int64 [records, 2], the stats block or None)"""
    tab.finish()
    cases = to_dev(tab.cases)
    arena = torch.as_tensor(tab.prefill(), device=DEV)
    out_dt = sc.OUT1 if fn == "pcc_test_send1" else sc.OUT2
    out = torch.full((tab.n * out_dt.itemsize,), 0xFF, dtype=torch.uint8, device=DEV)
    trace = torch.as_tensor(tab.trace_arr, device=DEV) if tab.trace else None
    stats = torch.zeros(L.pcc_test_send_stat_slots(), dtype=torch.int64, device=DEV) if profile else None
    rc = getattr(L, fn)(variant, 1 if tab.trace else 0, cases.data_ptr(), tab.n, arena.data_ptr(), tab.arena_records,
                        trace.data_ptr() if tab.trace else None, len(tab.trace_arr) if tab.trace else 0, tab.max_packets, sc.KEY0, sc.KEY1,
                        stats.data_ptr() if profile else None, out.data_ptr(), torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    assert rc == 0, "HIP error %d" % rc
    torch.cuda.synchronize()
    return (np.frombuffer(out.cpu().numpy().tobytes(), dtype=out_dt), arena.cpu().numpy().view(np.int64),
            stats.cpu().numpy() if profile else None)


def check(tab, got, arena, senders):
    """state, cursors and flags of every case; then every record of the arena, the untouched ones included"""
    want = tab.want
    for k in ("sent", "a", "d", "flags", "t", "tu", "q"):
        g, w = got[k].astype(np.int64).reshape(tab.n, -1), want[k].astype(np.int64).reshape(tab.n, -1)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, "%s of %d cases differ, first: case %d (%s) got %s want %s; its case: %s" % (
            k, bad.size, bad[0], tab.sub[bad[0]], g[bad[0]], w[bad[0]], tab.cases[bad[0]])
    wa = tab.want_arena().view(np.int64)
    if not np.array_equal(arena, wa):
        r = int(np.flatnonzero((arena != wa).any(axis=1))[0])
        offs = tab.ring_off.reshape(-1)
        k = int(np.searchsorted(offs, r, side="right")) - 1
        c, s = (k, 0) if senders == 1 else divmod(k, 2)
        cap = int(tab.cap.reshape(-1)[k])
        rel = r - int(offs[k])
        where = "accepted slot %d" % rel if rel < cap else "dropped slot %d" % (rel - cap) if rel < 3 * cap else "guard record %d behind the ring" % (rel - 3 * cap)
        raise AssertionError("record %d of the arena differs: case %d (%s) sender %d, %s (cap %d): got %s want %s; its case: %s" % (
            r, c, tab.sub[c], s, where, cap, arena[r].view(np.float64), wa[r].view(np.float64), tab.cases[c]))


def reach(dev, mirror, what):
    for k in mirror:
        assert 2 * dev[k] >= mirror[k], "%s: the device's closed forms carry %d packets of regime %s, the mirror commits %d: %s vs %s" % (
            what, dev[k], k, mirror[k], dev, mirror)


@pytest.mark.parametrize("build", ["plain", "profile"])
@pytest.mark.parametrize("entry", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(sc.CLASSES1))
def test_one_sender_passes_equal_the_plain_recurrence(harness, name, entry, build):
    variant, lanes = VARIANTS[entry]
    tab = sc.CLASSES1[name](lanes)
    got, arena, stats = launch(harness[build], "pcc_test_send1", variant, tab, build == "profile")
    check(tab, got, arena, 1)
    if build == "profile":
        counts, same = tab.mirror()
        assert same
        dev = counted(harness[build], stats, WHICH_TEAM if entry == "team" else WHICH1)
        serial = dev.pop("serial")
        mirror = {k: int(counts[:, col].sum()) for k, col in MIRROR_COLS1.items()}
        REPORT["%s/%s" % (name, entry)] = {"cases": tab.n, "packets": int(tab.npk.sum()), "device": dev, "mirror": mirror,
                                           "device_serial_or_chain": serial,
                                           "mirror_serial_or_chain": int(counts[:, [sc.PK_S, sc.PK_CHAIN]].sum())}
        reach(dev, mirror, "%s/%s" % (name, entry))


@pytest.mark.parametrize("build", ["plain", "profile"])
@pytest.mark.parametrize("staged", [0, 1])
@pytest.mark.parametrize("name", sorted(sc.CLASSES2))
def test_two_sender_passes_equal_the_plain_merged_recurrence(harness, name, staged, build):
    tab = sc.CLASSES2[name]()
    got, arena, stats = launch(harness[build], "pcc_test_send2", staged, tab, build == "profile")
    check(tab, got, arena, 2)
    if build == "profile":
        counts, same = tab.mirror()
        assert same
        got2 = counted(harness[build], stats, WHICH2)
        dev = {"token": got2["token"], "sweeps": got2["sweep256"] + got2["sweep64"]}
        mirror = {"token": int(counts[:, 1].sum()), "sweeps": int(counts[:, 3].sum() + counts[:, 5].sum())}
        REPORT["%s/%s" % (name, "staged2" if staged else "wave2")] = {"cases": tab.n, "packets": int(tab.npk.sum()), "device": dev, "mirror": mirror,
                                                                     "device_plain": got2["plain"], "mirror_plain": int(counts[:, 7].sum())}
        reach(dev, mirror, name)


def test_refused_cases_keep_their_prefill(harness):
    """the device validates a case before it touches memory: a ring outside the arena, a cap that is no power of two, a gap of 0,
    an interval beyond the packet cap, a NaN end, a trace row outside the trace -- skipped, outputs and arena left as they were --
    next to good cases of the same launch, which are sent as ever"""
    tab = sc.trace_overrun(64)
    tab.finish()
    keep = tab.cases.copy()
    bad = {0: ("ring_off", tab.arena_records), 8: ("cap", 96), 16: ("gap", 0.0), 24: ("end", 1e9), 32: ("end", float("nan")),
           40: ("trace_off", len(tab.trace_arr)), 48: ("cap", 32), 56: ("trace_stride", -1)}
    try:
        for c, (k, v) in bad.items():
            tab.cases[k][c] = v
        for variant in (0, 1, 2):
            got, arena, _ = launch(harness["plain"], "pcc_test_send1", variant, tab, False)
            raw = got.view(np.uint8).reshape(tab.n, -1)
            wa = tab.prefill().view(np.int64)
            good = np.array([c not in bad for c in range(tab.n)])
            for c in bad:
                assert (raw[c] == 0xFF).all(), (variant, c)
            for k in ("sent", "a", "d", "flags", "t", "tu", "q"):
                assert (got[k][good].astype(np.int64) == tab.want[k][good].astype(np.int64)).all(), (variant, k)
            full = tab.want_arena().view(np.int64)
            for c in range(tab.n):
                lo, hi = int(tab.ring_off[c]), int(tab.ring_off[c] + 3 * tab.cap[c])
                assert np.array_equal(arena[lo:hi], (wa if c in bad else full)[lo:hi]), (variant, c)
    finally:
        tab.cases[:] = keep
    L = harness["plain"]
    assert L.pcc_test_send1(0, 0, None, 1, None, 1, None, 0, 1, 0, 0, None, None, None) == 1       # hipErrorInvalidValue, nothing launched
    assert L.pcc_test_send1(3, 0, 1, 1, 1, 64, None, 0, 4096, 0, 0, None, 1, None) == 1
    assert L.pcc_test_send1(0, 0, 1, 1, 1, 64, None, 0, 1 << 20, 0, 0, None, 1, None) == 1
    assert L.pcc_test_send2(0, 1, 1, 1, 1, 64, None, 0, 4096, 0, 0, None, 1, None) == 1
