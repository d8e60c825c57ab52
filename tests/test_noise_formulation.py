"""The heap-free restatement of USE_LATENCY_NOISE (tests/models/noise_sorting_model.py, the numpy design study of pcc_noise_sorted.hip: counts, two sorts and a scan per interval)
against the oracle's event loop: every observation, reward, count and clock bit for bit.  CPU only."""
import numpy as np
import pytest

from oracle.pcc_oracle_py import PyOracleEnv
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "models"))
from noise_sorting_model import SortedNoiseEnv   # noqa: E402


def equal_time_pairs(heap):
    """Events of the oracle's heap whose time another event of the heap has too: len - distinct times."""
    times = [ev[0] for ev in heap]
    return len(times) - len(set(times))


def run_pair(seed, n_steps, scale=1.0, fixed=None, noise=1.1, ties=None):
    a = PyOracleEnv(seed=seed, latency_noise=noise, fixed=fixed)
    b = SortedNoiseEnv(seed=seed, latency_noise=noise, fixed=fixed)
    oa, ob = a.reset(), b.reset()
    assert np.array_equal(oa, ob)
    acts = np.random.RandomState(seed).uniform(-1, 1, n_steps) * scale
    for t in range(n_steps):
        if ties is not None:
            ties.append(equal_time_pairs(a.heap))
        oa, ra, da, _ = a.step(acts[t])
        ob, rb, db, _ = b.step(acts[t])
        assert (a.sent, a.acked, a.lost) == (b.sent, b.acked, b.lost), (seed, t)
        assert a.now == b.now and a.q == b.q and a.tq == b.tq, (seed, t)
        assert a.rtts[0] == b.rtts[0], (seed, t)
        assert np.array_equal(oa, ob) and ra == rb and da == db, (seed, t)
        assert a.draws == b.draws, (seed, t)
    return b


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 7])
def test_random_links_match_the_event_loop(seed):
    run_pair(seed, 120)


def test_rates_pushed_up_and_down_match_and_the_blocks_are_wide():
    b = run_pair(11, 150, scale=8.0)                     # large actions: rates from the floor to the ceiling
    b = run_pair(5, 100, fixed=(400.0, 0.3, 2000, 0.02, 900.0))   # a fast sender on a long link: many packets in flight
    assert max(b.block_sizes) >= 100                      # hundreds of SENDs with no dependence on each other


def test_lossy_shallow_queue_matches():
    run_pair(3, 100, fixed=(150.0, 0.08, 2, 0.04, 200.0))


# ---- one or two senders on the link (tests/models/noise_sorting2_model.py)
from noise_sorting2_model import SortedNoiseEnvS   # noqa: E402


def run_pair_s(seed, n_steps, n_senders, scale=1.0, fixed=None, noise=1.1, ties=None):
    a = PyOracleEnv(seed=seed, latency_noise=noise, fixed=fixed, n_senders=n_senders)
    b = SortedNoiseEnvS(seed=seed, latency_noise=noise, fixed=fixed, n_senders=n_senders)
    oa, ob = a.reset(), b.reset()
    assert np.array_equal(oa, ob)
    acts = np.random.RandomState(seed).uniform(-1, 1, (n_steps, n_senders)) * scale
    for t in range(n_steps):
        if ties is not None:
            ties.append(equal_time_pairs(a.heap))
        act = acts[t] if n_senders > 1 else acts[t, 0]
        oa, ra, da, _ = a.step(act)
        ob, rb, db, _ = b.step(act)
        assert (a.sent, a.acked, a.lost) == (b.sent, b.acked, b.lost), (seed, t)
        assert a.now == b.now and a.q == b.q and a.tq == b.tq, (seed, t)
        assert a.rtts == b.rtts, (seed, t)
        assert np.array_equal(oa, ob) and ra == rb and da == db, (seed, t)
        assert a.draws == b.draws, (seed, t)
    return b


@pytest.mark.parametrize("seed", [0, 1, 4])
def test_two_senders_match_the_event_loop(seed):
    run_pair_s(seed, 100, 2)


def test_two_senders_large_actions_and_a_fast_pair_on_a_long_link():
    run_pair_s(9, 120, 2, scale=8.0)
    b = run_pair_s(6, 80, 2, fixed=(450.0, 0.3, 3000, 0.01, 700.0, 300.0))
    assert max(b.block_sizes) >= 100


def test_the_general_restatement_with_one_sender():
    run_pair_s(2, 100, 1)


# ---- MAX_LATENCY_NOISE off the reference's 1.1 (include/pcc_sim.h: pcc_set_latency_noise takes [1, 16])
# The golden vectors tie both oracles to the unmodified reference at 1.1 only.  Off 1.1 the reference of the device tests
# (tests/test_noise_domain.py) is that independent restatements agree: the Python oracle's event loop against the two
# sorting models here, and against the C oracle in tests/test_oracle_settings_cpu.py.
#   1.0: noise_span == 0 -- the draws are still consumed, every factor is exactly 1, and event times tie exactly;
#   2, 16: a packet takes up to 16 times its latency and overtakes hundreds of others.
# Links on which events tie at 1.0 (bw, dl, queue, loss, rate0...): every quantity a power of two or a small multiple, so
# that with zero actions 1 / rate, dl and 1 / bw add up without rounding.
TIE_LINKS_1 = [(64.0, 0.125, 8, 0.0, 64.0), (64.0, 0.125, 8, 0.0, 128.0), (128.0, 0.25, 4, 0.25, 256.0)]
TIE_LINKS_2 = [(64.0, 0.125, 8, 0.0, 64.0, 64.0), (128.0, 0.25, 4, 0.25, 256.0, 128.0)]


@pytest.mark.parametrize("noise", [1.0, 2.0, 16.0])
def test_random_links_off_the_reference_noise_match_the_event_loop(noise):
    for seed in (0, 3):
        run_pair(seed, 30, noise=noise)
    run_pair(11, 30, scale=8.0, noise=noise)


@pytest.mark.parametrize("noise", [1.0, 2.0, 16.0])
def test_two_senders_off_the_reference_noise_match_the_event_loop(noise):
    run_pair_s(1, 30, 2, noise=noise)
    run_pair_s(9, 30, 2, scale=8.0, noise=noise)
    run_pair_s(2, 30, 1, noise=noise)


@pytest.mark.parametrize("fixed", TIE_LINKS_1)
def test_links_that_tie_at_noise_one_match_and_do_tie(fixed):
    """Zero actions (1 / rate stays dyadic) at MAX_LATENCY_NOISE = 1.0: the oracle's heap holds events of equal time at the start
    of the steps -- a 1.0 case without ties would test nothing -- and both restatements order them as the event loop does."""
    for model in (run_pair, lambda *a, **k: run_pair_s(a[0], a[1], 1, **k)):
        ties = []
        model(0, 25, scale=0.0, fixed=fixed, noise=1.0, ties=ties)
        assert sum(ties) >= 25 and sum(1 for n in ties if n) >= 10, ties


@pytest.mark.parametrize("fixed", TIE_LINKS_2)
def test_two_sender_links_that_tie_at_noise_one_match_and_do_tie(fixed):
    ties = []
    run_pair_s(0, 25, 2, scale=0.0, fixed=fixed, noise=1.0, ties=ties)
    assert sum(ties) >= 25 and sum(1 for n in ties if n) >= 10, ties


def tie_actions(n, T, n_senders, seed, shares):
    """The actions of tests/test_noise_domain.py's tie cases, for delta_scale = 0.5: zero for the first ten steps; then, for the
    first half of each of the batch's `shares` (one per link), +-2 or 0 -- d = +-1 exactly, the rate doubles or halves and 1 / rate
    stays a power of two until a clamp at 40 or 1000 ends that -- and U(-1, 1) for the other half.  [n, T] or [n, T, S]."""
    rs = np.random.RandomState(seed)
    a = rs.uniform(-1, 1, (n, T, n_senders))
    dyadic = rs.choice([-2.0, 0.0, 0.0, 2.0], (n, T, n_senders))
    share = n // shares
    first_half = (np.arange(n) % share) < share // 2
    a[first_half] = dyadic[first_half]
    a[:, :10] = 0.0
    return a[:, :, 0] if n_senders == 1 else a


@pytest.mark.parametrize("n_senders", [1, 2])
def test_the_tie_actions_keep_the_events_tied_after_the_tenth_step(n_senders):
    """What tests/test_noise_domain.py feeds the device at 1.0: on each dyadic link, one env with the doubling / halving actions
    and one with random ones, at delta_scale = 0.5.  Events of equal time at the start of every one of the steps 0..9, and at
    the start of a third or more of the later ones (dl is dyadic whatever the rate does)."""
    links = TIE_LINKS_1 if n_senders == 1 else TIE_LINKS_2
    n, T = 8 * len(links), 30
    acts = tie_actions(n, T, n_senders, 24, shares=len(links))
    for k, fixed in enumerate(links):
        later = 0
        for i in (8 * k, 8 * k + 2, 8 * k + 4):      # two of the share's first half, one of its second
            env = PyOracleEnv(seed=i, fixed=fixed, n_senders=n_senders, ctor_draws=0, delta_scale=0.5, latency_noise=1.0)
            env.reset()
            ties = []
            for t in range(T):
                ties.append(equal_time_pairs(env.heap))
                env.step(acts[i, t])
            assert min(ties[:10]) >= 1, (fixed, i, ties)
            later += sum(1 for x in ties[12:] if x)
        assert later >= 18, (fixed, later)      # (of 3 x 18 step starts: the ties do not end with the zero actions)
