"""The reach audit of the send half's parity tests.

Every send path is exact and the tuning only chooses which one runs -- so a parity test whose docstring says "regime C of
the wave passes" or "the token pass's home ground" still passes, number for number, when a threshold or a precondition has
moved and its envs fall through to the serial pass or the lane rounds.  This file runs those parity tests THEMSELVES (their
own inputs, by construction) on the profile build (-DPCC_PROFILE=1, libpcc_sim_prof.so: the per-path counters of
pcc_debug_path_stats, include/pcc_sim.h), one child process per slice, and holds two things:
  * the profile build reproduces the oracle and the goldens bit for bit on every audited case (the library every figure of
    tools/ comes from was never compared with anything before), and
  * the path each test names carried packets: the table REACH below, one row per label, each condition taken from the claim
    written in the parity test.  `> 0` rows also carry a cap on what the test may leave uncovered: the named path carries at
    least a quarter of the case's packets (QUARTER) -- except where the path structurally cannot, which the row says with the
    share measured when it was written (profiles/r21_path_reach.json has every label's counters; they are a record, not
    thresholds).  The two-sender token-pass labels have a floor of their own: the kernel's token-pass share of the packets
    is at least half the share the CPU model of the pass (tests/models/send_pass2_model.c) commits by token pass on its own
    fuzz.
tests/test_gpu_parity.py calls _reach(env, label) before it closes an audited handle; the call does nothing unless
PCC_REACH_OUT names a file.  PCC_REACH_RECORD=<file> makes this module write what it measured there (the record under
profiles/ was made that way).  Cost: the three children take 18 + 14 + 9 s, the file 44 s; the same 45 parity tests take 31 s
in one process on the product build."""
import ctypes
import json
import os
import re
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUARTER = 0.25

# ---- the slices: -k expressions over tests/test_gpu_parity.py, one child process each, one at a time
SLICES = {
    "one_sender": "queue_limits_just_above or test_wave_path_on_golden_traces or team_path_on_golden_traces or send_paths_are_exact",
    "two_senders": "two_sender_token_pass or two_sender_wave_path or two_sender_philox_batches",
    "recorded_only": "long_drop_runs or edge_links or philox_batches_with_odd_shapes",
}
SLICE_TIMEOUT = 540   # seconds, per child: inside the ten minutes every GPU test has (tests/conftest.py)

# ---- groups of counters (names of BatchedNetworkEnv.PATH_STAT_NAMES)
REGIMES = ("a", "b_scan", "b_free", "c")
CLOSED64_PK = tuple("%s_packets" % r for r in REGIMES)                                   # 64-lane closed-form passes
WAVE64_PASSES = tuple("%s_passes" % r for r in REGIMES) + ("serial_passes",)             # every pass of a lone wavefront
WAVE64_PK = CLOSED64_PK + ("serial_packets",)
TEAM_PASSES = tuple("team_%s_passes" % r for r in REGIMES) + ("team_serial_passes",)
TEAM_PK = tuple("team_%s_packets" % r for r in REGIMES) + ("team_serial_packets",)
TWO_PASSES = ("two_token_passes", "two_sweep256_passes", "two_sweep64_passes", "two_plain_passes", "two_chain_passes")
TWO_PK = tuple(n.replace("_passes", "_packets") for n in TWO_PASSES)
SWEEP_PASSES = ("two_sweep256_passes", "two_sweep64_passes")
SWEEP_PK = ("two_sweep256_packets", "two_sweep64_packets")
LANE_PK = ("lane_round_packets",)
EVERY_WAVE_PASS = WAVE64_PASSES + TEAM_PASSES + TWO_PASSES + ("envs_heavy", "envs_team", "envs_taken_over")


def zero(what, *names):
    return ("zero", what, names)


def some(what, *names):
    """> 0, a counter of passes, envs or refusals: no share of the packets goes with it"""
    return ("some", what, names)


def carries(what, *names, **kw):
    """> 0 packets, and at least `floor` (default: a quarter) of the case's packets (the handle's total_sent).  floor=None: the
    path structurally cannot carry a quarter -- `why` says so, with its share when the row was written."""
    return ("carries", what, names, kw.get("floor", QUARTER), kw.get("why"))


TOKEN_FLOOR = "token"   # (resolved at run time: half the CPU model's token-pass share on its own fuzz)
PARITY = "test_gpu_parity.py"
Q, TOK = "test_queue_limits_just_above_a_power_of_two_match_oracle", "test_two_sender_token_pass_matches_oracle"
TUNE, TWO = "test_send_paths_are_exact_whatever_the_tuning", "test_two_sender_philox_batches_match_oracle"
WAVE_G, TEAM_G = "test_wave_path_on_golden_traces", "test_team_path_on_golden_traces"

# ---- the table: (test, label) -> conditions.  A label of tests/test_gpu_parity.py is the knob set ("name=value, ...") or the golden.
# What the first run of this audit found, and what became of it (the knob sets below are the mended ones):
#   * "lane-round packets == 0" cannot hold for any handle: the step after a reset has no work lists yet, and heavy_predict /
#     team_predict choose a path through the lists -- that one interval goes by lane rounds whatever the knobs say (1.3 % of the
#     packets of the tuning case, 0.4 % of the power-of-two case).  The rows ask for it where the knob acts: no lane-round packet
#     in a launch that walks the lists (LISTED_LANE_PK).  The parity tests' docstrings said "from the first interval on".
#   * the lanes that list-less step hands over (takeover_lanes = 1 by default) go to a lone wavefront: the "every env a team
#     item" cases had a dozen 64-lane passes; they now run with takeover_lanes=0.
#   * test_wave_path_on_golden_traces ("every env handed to the heavy wavefront") sent 54 % / 99.5 % of saturating_0_2 /
#     fixed_deepq by TEAM passes: it now sets team_predict=1e18.
#   * test_two_sender_philox_batches_match_oracle[takeover_lanes=0] ("lane-serial only") sent 72 % of its packets by the wave
#     path, as heavy items: it now sets heavy_predict=1e18 as well.
#   * "lane rounds, wave passes and team passes side by side" (heavy_predict=16, team_predict=100) was 1.4 % / 1.1 % / 97.5 %:
#     the thresholds now cut the case's packets into about thirds.
LISTED_LANE_PK = ("lane_round_listed_packets",)
REACH = {}
# "Regime C of the wave passes ... half of them sent one env per wavefront"
REACH[(Q, "defaults")] = [some("regime-C passes", "c_passes"), carries("regime C", "c_packets")]
REACH[(Q, "heavy_predict=0, team_predict=1e+18, heavy_item_packets=0")] = [
    some("regime-C passes", "c_passes"), carries("regime C", "c_packets"), zero("lane rounds of listed launches", *LISTED_LANE_PK),
    zero("team passes", *TEAM_PASSES)]
# "the closed-form pass of the two-sender wave path ... every env sent by the wave path"
for case in ("overdriven", "edges", "mixed"):
    for label in ("heavy_predict=0", "takeover_lanes=64, round_packets=8"):
        REACH[("%s[%s]" % (TOK, case), label)] = [some("token passes", "two_token_passes"),
                                                  carries("the token pass", "two_token_packets", floor=TOKEN_FLOOR)]
        if case == "edges":   # "its preconditions break and hold by turns"
            REACH[("%s[%s]" % (TOK, case), label)] += [some("token passes refused", "two_refused_time", "two_refused_queue"),
                                                       some("sweep passes", *SWEEP_PASSES)]
REACH[("test_two_sender_wave_path_across_powers_of_two_in_time_matches_oracle", "")] = [
    some("token or sweep passes", "two_token_passes", *SWEEP_PASSES), carries("token and sweep passes", "two_token_packets", *SWEEP_PK)]
REACH[("test_two_sender_wave_path_on_golden_trace", "")] = [carries("the two-sender wave path", *TWO_PK)]
for name in ("saturating_0_2", "fixed_deepq"):
    REACH[(WAVE_G, name)] = [carries("64-lane closed-form passes", *CLOSED64_PK), zero("team passes", *TEAM_PASSES)]
REACH[(WAVE_G, "fixed_lossy")] = [
    carries("64-lane closed-form passes", *CLOSED64_PK, floor=None,
            why="half of this link's packets are lost at random: the sender is faster than the link (400 against 300 packets/s), so regime "
                "A does not apply, and the queue sees 200 packets/s and keeps running empty, so regime B is refused or stops after a "
                "few packets -- 94 % of the packets go by the serial pass; closed forms carried 0.021 of them when this was written"),
    carries("64-lane passes", *WAVE64_PK), zero("team passes", *TEAM_PASSES)]
for name in ("saturating_0_2", "fixed_deepq", "fixed_lossy", "default_pm1"):
    REACH[(TEAM_G, name)] = [some("team passes", *TEAM_PASSES), carries("team passes", *TEAM_PK), zero("64-lane passes", *WAVE64_PASSES)]
# the knob comments of test_send_paths_are_exact_whatever_the_tuning
REACH[(TUNE, "takeover_lanes=64, round_packets=8")] = [some("envs taken over from lane rounds", "envs_taken_over"),
                                                      carries("the wave path", *WAVE64_PK + TEAM_PK)]
REACH[(TUNE, "takeover_lanes=0, heavy_predict=1e+18")] = [zero("every wave-pass counter", *EVERY_WAVE_PASS), carries("lane rounds", *LANE_PK)]
REACH[(TUNE, "heavy_predict=0")] = [zero("lane rounds of listed launches", *LISTED_LANE_PK), carries("the wave path", *WAVE64_PK + TEAM_PK)]
REACH[(TUNE, "heavy_predict=0, team_predict=0, takeover_lanes=0")] = [
    some("team passes", *TEAM_PASSES), carries("team passes", *TEAM_PK), zero("64-lane passes", *WAVE64_PASSES),
    zero("lane rounds of listed launches", *LISTED_LANE_PK)]
REACH[(TUNE, "team_predict=1e+18")] = [zero("team passes", *TEAM_PASSES), zero("team items", "envs_team")]
REACH[(TUNE, "heavy_predict=470, team_predict=1800, round_packets=16")] = [   # "lane rounds, wave passes and team passes side by side"
    carries("lane rounds", *LANE_PK), carries("64-lane passes", *WAVE64_PK), carries("team passes", *TEAM_PK)]
# "nearly everything by wave passes of every regime": these inputs reach all four closed forms and the serial pass -- every one is required
REACH[(TUNE, "heavy_predict=16, round_packets=16")] = [
    carries("wave passes", *WAVE64_PK + TEAM_PK), some("regime A", "a_passes"), some("regime B with the scan", "b_scan_passes"),
    some("regime B without it", "b_free_passes"), some("regime C", "c_passes"), some("the serial pass", "serial_passes")]
# the knob comments of test_two_sender_philox_batches_match_oracle
REACH[(TWO, "takeover_lanes=0, heavy_predict=1e+18")] = [zero("two-sender wave passes", *TWO_PASSES), zero("wave-path items", "envs_heavy", "envs_taken_over"),
                                                        carries("lane rounds", *LANE_PK)]
REACH[(TWO, "takeover_lanes=64, round_packets=8")] = [some("two-sender wave passes", *TWO_PASSES), carries("the two-sender wave path", *TWO_PK)]
REACH[(TWO, "takeover_lanes=64, round_packets=4, heavy_predict=200")] = [some("two-sender wave passes", *TWO_PASSES),
                                                                        carries("the two-sender wave path", *TWO_PK)]
RECORDED_ONLY = ("test_long_drop_runs_match_oracle", "test_edge_links_match_oracle", "test_philox_batches_with_odd_shapes_match_oracle")


def _key(rec):
    return (re.sub(r"\[knobs\d+\]$", "", rec["test"]), rec["label"])


def _total(rec):
    """the packets in the send paths' counters: total_sent less what the retire half sends itself (the SEND events its event loop
    meets, pcc_retire_env.h: in no send path's counter) -- the same remainder for every knob set of a case"""
    p = rec["path"]
    return sum(p[n] for n in LANE_PK + WAVE64_PK + TEAM_PK + TWO_PK)


def _check(rec, conds, token_floor):
    """-> the conditions of one record, evaluated"""
    p, total, rows = rec["path"], max(1, rec["total_sent"]), []
    for c in conds:
        kind, what, names = c[0], c[1], c[2]
        value = sum(p[n] for n in names)
        share, floor, note = None, None, None
        if kind == "zero":
            met = value == 0
        elif kind == "some":
            met = value > 0
        else:
            share, floor, note = value / total, c[3], c[4]
            if floor == TOKEN_FLOOR:
                floor = token_floor
            met = value > 0 and (floor is None or share >= floor)
        rows.append({"what": what, "kind": kind, "value": value, "share": share, "floor": floor, "met": bool(met), "exception": note})
    return rows


@pytest.fixture(scope="module")
def model_token_share():
    """The share of its packets the CPU model of the token pass (256 positions: 64 lanes x 4) commits by token pass on its own
    fuzz -- the run of tests/test_send_pass_model.py::test_two_sender_token_pass_model[64-4]."""
    src = os.path.join(ROOT, "tests", "models", "send_pass2_model.c")
    lib = os.path.join(ROOT, "tests", "models", "libsend_pass2_model.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", lib, "-lm"])
    L = ctypes.CDLL(lib)
    L.pcc_model2_fuzz.restype = ctypes.c_long
    L.pcc_model2_fuzz.argtypes = [ctypes.c_long, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    assert L.pcc_model2_set_shape(64, 4) == 0
    stats = (ctypes.c_uint64 * 4)()
    assert L.pcc_model2_fuzz(6000, 777 + 4, stats) == 0
    return int(stats[1]) / float(int(stats[1]) + int(stats[2]))


class Audit(object):
    """The slices' children, each run once, on demand (so that each runs inside the time limit of the test that asks for it),
    one at a time; after a child that failed, faulted or ran into its time limit no other is started."""

    def __init__(self, tmp, model_token_share):
        self.tmp, self.model_token_share = tmp, model_token_share
        self.slices, self.records, self.stopped = {}, [], None

    def codes(self):
        return {k: v["returncode"] for k, v in self.slices.items()}

    def need(self, name):
        if name in self.slices:
            return self.slices[name]
        assert self.stopped is None, "slice %s not run: slice %s failed before it (%s)" % (name, self.stopped, self.codes())
        reach_out = str(self.tmp / (name + ".jsonl"))
        envv = dict(os.environ, PCC_DEBUG_TIMELINE="2", PCC_REACH_OUT=reach_out)
        envv.pop("PCC_SIM_LIBRARY", None)
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", PARITY), "-m", "gpu", "-x", "-q", "-k", SLICES[name],
                                "-p", "no:cacheprovider"], cwd=ROOT, env=envv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               universal_newlines=True, timeout=SLICE_TIMEOUT)
            rc, tail = r.returncode, r.stdout[-3000:]
        except subprocess.TimeoutExpired as e:
            rc, tail = "timeout", e.stdout[-3000:] if isinstance(e.stdout, str) else ""
        sl = {"returncode": rc, "tail": tail, "seconds": round(time.time() - t0, 1), "records": 0}
        self.slices[name] = sl
        if rc != 0:
            self.stopped = name
        if os.path.exists(reach_out):
            with open(reach_out) as f:
                recs = [json.loads(line) for line in f if line.strip()]
            for rec in recs:
                rec["slice"] = name
                tot = max(1, rec["total_sent"])
                pk = lambda names: sum(rec["path"][n] for n in names) / tot
                rec["packets_by_path"] = _total(rec)
                rec["shares"] = {"lane_rounds": pk(LANE_PK), "wave64": pk(WAVE64_PK), "team": pk(TEAM_PK), "two_sender_wave": pk(TWO_PK),
                                 "regime_c": pk(("c_packets",)), "two_token": pk(("two_token_packets",)), "two_sweeps": pk(SWEEP_PK)}
                rec["conditions"] = _check(rec, REACH.get(_key(rec), []), 0.5 * self.model_token_share)
            sl["records"] = len(recs)
            self.records += recs
        self.write_record()
        return sl

    def write_record(self):
        record = os.environ.get("PCC_REACH_RECORD")
        if not record:
            return
        import pcc_rl_amd.build as pbuild
        doc = {"what": "tests/test_path_reach.py: the per-path counters (pcc_debug_path_stats) of every audited label of tests/test_gpu_parity.py "
                       "on the profile build, the share of the case's packets each path carried and the conditions of the table REACH",
               "build": pbuild.build_info(pbuild.library_path(True)), "model_token_share": self.model_token_share,
               "token_floor": 0.5 * self.model_token_share,
               "slices": {k: {kk: vv for kk, vv in v.items() if kk != "tail"} for k, v in self.slices.items()},
               "records": self.records}
        with open(record, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)


def _slice_of(test):
    base = test.split("[")[0]
    return "one_sender" if base in (Q, WAVE_G, TEAM_G, TUNE) else "recorded_only" if base in RECORDED_ONLY else "two_senders"


@pytest.fixture(scope="module")
def audit(tmp_path_factory, model_token_share):
    """The profile library is built once, before the first child."""
    import pcc_rl_amd
    pcc_rl_amd.build_library(profile=True)
    return Audit(tmp_path_factory.mktemp("reach"), model_token_share)


@pytest.mark.parametrize("name", list(SLICES))
def test_profile_build_matches_the_oracle_on_the_audited_cases(audit, name):
    """The slice of the parity file on libpcc_sim_prof.so: bit for bit against the oracle and the goldens, counters on."""
    sl = audit.need(name)
    print("slice %s: %.1f s, %d records" % (name, sl["seconds"], sl["records"]))
    assert sl["returncode"] == 0, "slice %s on the profile build (%s):\n%s" % (name, sl["returncode"], sl["tail"])
    assert " passed" in sl["tail"] and "no tests ran" not in sl["tail"] and " failed" not in sl["tail"], sl["tail"]
    assert sl["records"] > 0, "the slice left no counters: _reach() was not called"


@pytest.mark.parametrize("key", sorted(REACH), ids=lambda k: "%s|%s" % k)
def test_named_path_is_reached(audit, key):
    """The row of REACH for one label: every record of that label meets every condition of the row."""
    audit.need(_slice_of(key[0]))
    recs = [r for r in audit.records if _key(r) == key]
    assert recs, "no counters for %s: the label is gone from tests/test_gpu_parity.py, or its slice failed (%s)" % (key, audit.codes())
    for rec in recs:
        for c in rec["conditions"]:
            print("%s | %s: %s %s = %d%s" % (key[0], key[1], c["kind"], c["what"], c["value"],
                                           "" if c["share"] is None else ", share %.4f (floor %s)" % (c["share"], c["floor"])))
        missed = [c for c in rec["conditions"] if not c["met"]]
        assert not missed, "%s | %s: %s\ncounters: %s" % (key[0], key[1], missed, rec["path"])
        # no packet is in two paths' counters (see _total for those in none)
        assert 0 < rec["packets_by_path"] <= rec["total_sent"], (rec["packets_by_path"], rec["total_sent"])


def test_every_audited_label_is_in_the_table_or_recorded_only(audit):
    """A label the parity file gains (a new knob set, a new golden) needs a row, or a place among the recorded-only tests."""
    for name in SLICES:
        assert audit.need(name)["returncode"] == 0, audit.codes()
    # the same inputs under other knobs: the same packets in the send paths' counters, however they are spread over the paths
    by_input = {}
    for rec in audit.records:
        by_input.setdefault((rec["n_envs"], rec["n_senders"], rec["total_sent"]), set()).add(rec["packets_by_path"])
    assert all(len(v) == 1 for v in by_input.values()), {k: v for k, v in by_input.items() if len(v) > 1}
    assert sum(1 for rec in audit.records if rec["n_senders"] == 1) >= 27 and sum(1 for rec in audit.records if rec["n_senders"] == 2) >= 15
    retire_side = {"retire_wide_predict=0", "retire_wide_predict=1e+18", "retire_wide_predict=40, heavy_predict=64"}   # (no send path named)
    unnamed = {"send_envs_per_wave=7, round_packets=64, takeover_lanes=3", "send_waves=1, heavy_predict=64", "send_waves=32, heavy_predict=64",
               "send_envs_per_wave=64, heavy_predict=256, takeover_lanes=8", "heavy_predict=64, team_predict=64, send_waves=1",
               "heavy_predict=32, heavy_item_packets=0", "heavy_predict=32, heavy_item_packets=1e+06, team_predict=1e+18",
               "defaults", "heavy_predict=100, send_waves=2"}   # (launch shapes and item sizes: their comments name no path)
    for rec in audit.records:
        k = _key(rec)
        base = k[0].split("[")[0]
        assert k in REACH or base in RECORDED_ONLY or (base in (TUNE, TWO) and k[1] in retire_side | unnamed), k
