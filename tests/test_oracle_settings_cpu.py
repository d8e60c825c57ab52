"""The oracle's own settings moved off their defaults, on the CPU: the sampling ranges (OracleEnv.set_ranges, run_batch(ranges=...)),
back from fixed links to sampling (clear_params), delta_scale, and actions that are infinite or overflow.  These are the inputs of
tests/test_settings_parity.py (which imports RANGE_SETS and the action helpers from here): what is checked here is that the
reference side of those comparisons is sound by itself -- the ranges reach the draws, nothing is NaN or infinite in any column --
before a device is asked to reproduce it."""
import math

import numpy as np
import pytest

import oracle

# (lo, hi) of (bandwidth pkt/s, one-way latency s, queue exponent x of queue = 1 + floor(e^x), loss probability, rate0 / bw)
RANGE_SETS = {
    # starting rates of 2 .. 240 pkt/s: neither the reference nor reset_env clamps rate0, so the two warm-up intervals of most
    # envs run below MIN_RATE (40); queues of 2 or 3 packets, up to nine packets in ten lost
    "slow_lossy_shallow": ((20.0, 0.01, 0.0, 0.3, 0.1), (60.0, 0.02, 1.0, 0.9, 4.0)),
    # lo == hi: one link for every env, and every packet lost -- no acknowledgement ever arrives
    "every_packet_lost": ((200.0, 0.03, 2.0, 1.0, 0.5), (200.0, 0.03, 2.0, 1.0, 0.5)),
    # queues of 22 027 .. 162 755 packets, intervals of a few milliseconds: many monitor intervals send one packet or none
    "fast_deep_short": ((1e4, 1e-3, 10.0, 0.0, 0.01), (2e4, 5e-3, 12.0, 0.0, 0.05)),
    # the reference's own ranges (ns:355-358), passed explicitly
    "default_explicit": ((100.0, 0.05, 0.0, 0.0, 0.3), (500.0, 0.5, 8.0, 0.05, 1.5)),
}


def actions(seed, n, T, n_senders=1):
    """U(-1, 1.5), the parity suite's usual actions: [n, T] or [n, T, S]."""
    return np.random.RandomState(seed).uniform(-1, 1.5, (n, T) if n_senders == 1 else (n, T, n_senders))


def extreme_rate_actions(seed, n, T):
    """U(-1, 1.5) with +inf, -inf, +1e308 and -1e308 in a few envs at a few steps (also twice in a row, and at the first step)."""
    a = actions(seed, n, T)
    big = (np.inf, -np.inf, 1e308, -1e308)
    for k, (i, t) in enumerate([(0, 0), (1, 0), (2, 1), (3, 1), (5, 7), (5, 8), (6, 7), (6, 8), (n - 1, T - 1), (n - 2, T - 2),
                                (n // 2, 3), (n // 2, 4), (n // 2 + 1, 3), (n // 2 + 1, 5)]):
        a[i, t] = big[k % 4]
    a[7, 10:14] = (np.inf, -np.inf, -1e308, 1e308)      # floor to ceiling and back inside one env
    return a


def finite(ref):
    return all(np.isfinite(ref[k]).all() for k in ("steps", "obs", "obs0", "params", "warm"))


def test_equal_bounds_give_every_env_the_link_that_set_params_gives():
    """lo == hi in all five ranges: a + (b - a) * u == a whatever u is, so every env has the same link -- and the run equals the one
    whose link was given through set_params (bw, dl, 1 + floor(e^x), loss, [f * bw]), every column of every env (the loss draws
    are keyed by env id and interval, not by how many parameter draws came before)."""
    n, T, seed = 24, 25, 3
    bw, dl, x, loss, f = 180.0, 0.07, 3.3, 0.03, 1.2
    a = actions(seed, n, T)
    got = oracle.run_batch(a, seed=seed, ranges=((bw, dl, x, loss, f), (bw, dl, x, loss, f)))
    queue = 1 + math.floor(math.exp(x))
    assert queue == 28
    assert (got["params"][:, [0, 1, 3, 4]] == np.array([bw, dl, loss, f * bw])).all()
    assert (np.round(got["params"][:, 2], 6) == queue).all()      # (reported as max_queue_delay * bw: an integer up to rounding)
    want = oracle.run_batch(a, seed=seed, params=np.tile([bw, dl, queue, loss, f * bw], (n, 1)))
    for k in ("steps", "obs", "obs0", "params", "warm"):
        assert np.array_equal(got[k], want[k]), k
    assert not np.array_equal(got["steps"][0], got["steps"][1])      # (the envs do differ: their own actions and loss draws)
    # two senders: one factor, two draws of it
    a2 = actions(seed, n, T, 2)
    got = oracle.run_batch(a2, n_senders=2, seed=seed, ranges=((bw, dl, x, loss, f), (bw, dl, x, loss, f)))
    want = oracle.run_batch(a2, n_senders=2, seed=seed, params=np.tile([bw, dl, queue, loss, f * bw, f * bw], (n, 1)))
    for k in ("steps", "obs", "obs0", "params", "warm"):
        assert np.array_equal(got[k], want[k]), k


def test_default_ranges_passed_explicitly_equal_no_call_at_all():
    n, T, seed = 24, 25, 4
    a = actions(seed, n, T)
    want = oracle.run_batch(a, seed=seed)
    got = oracle.run_batch(a, seed=seed, ranges=RANGE_SETS["default_explicit"])
    for k in ("steps", "obs", "obs0", "params", "warm"):
        assert np.array_equal(got[k], want[k]), k
    # ... and through the env object, which run_batch does not use
    o, p = oracle.OracleEnv(), oracle.OracleEnv()
    for e in (o, p):
        e.rng_philox(seed, 5)
    o.set_ranges(*RANGE_SETS["default_explicit"])
    assert np.array_equal(o.reset(), p.reset()) and np.array_equal(o.params(), p.params())
    assert np.array_equal(o.params()[:5], want["params"][5, :5])
    with pytest.raises(ValueError):
        o.set_ranges((1.0, 2.0), (3.0, 4.0))


def test_set_ranges_and_clear_params_apply_at_the_next_reset():
    """The env object's life cycle, as section 4 of the parity file drives it: a setter changes what the NEXT reset draws from and
    leaves the running episode alone; clear_params goes back from fixed links to sampling."""
    seed, gid = 9, 3
    lo, hi = RANGE_SETS["slow_lossy_shallow"]
    o, plain = oracle.OracleEnv(), oracle.OracleEnv()
    for e in (o, plain):
        e.rng_philox(seed, gid)
        e.reset()
    o.set_ranges(lo, hi)
    for t in range(5):      # the running episode goes on untouched
        a = 0.3 * t - 0.5
        o.step(a); plain.step(a)
        assert np.array_equal(o.last_row, plain.last_row)
    o.reset(); plain.reset()
    p = o.params()
    # (params()[2] is the queue as max_queue_delay * bw: an integer up to rounding)
    assert lo[0] <= p[0] <= hi[0] and lo[1] <= p[1] <= hi[1] and round(p[2], 6) in (2.0, 3.0) and lo[3] <= p[3] <= hi[3]
    assert lo[4] * p[0] <= p[4] <= hi[4] * p[0]
    # the same draw through another range: u = (bw - lo) / (hi - lo) on both sides (to the rounding of a + (b - a) * u)
    u_new, u_old = (p[0] - lo[0]) / (hi[0] - lo[0]), (plain.params()[0] - 100.0) / 400.0
    assert abs(u_new - u_old) < 1e-9
    # fixed links, then back: episode 3 of this env is episode 3 of an env that never had them
    o.set_params(150.0, 0.04, 7.0, 0.01, [90.0])
    o.reset()
    assert np.array_equal(o.params()[:5], [150.0, 0.04, 7.0, 0.01, 90.0])
    o.clear_params()
    o.reset()
    other = oracle.OracleEnv()
    other.rng_philox(seed, gid)
    other.set_ranges(lo, hi)
    for _ in range(4):
        other.reset()
    assert np.array_equal(o.params(), other.params())


@pytest.mark.parametrize("n_senders", [1, 2])
@pytest.mark.parametrize("name", sorted(RANGE_SETS))
def test_range_sets_run_finite_in_every_column(name, n_senders):
    n, T, seed = 96, 40, 12
    ref = oracle.run_batch(actions(seed, n, T, n_senders), n_senders=n_senders, seed=seed, ranges=RANGE_SETS[name])
    assert finite(ref), name
    lo, hi = RANGE_SETS[name]
    p = ref["params"]
    assert (p[:, 0] >= lo[0]).all() and (p[:, 0] <= hi[0]).all() and (p[:, 1] >= lo[1]).all() and (p[:, 1] <= hi[1]).all()
    assert (p[:, 2] >= 1 + math.floor(math.exp(lo[2])) - 1e-6).all() and (p[:, 2] <= 1 + math.floor(math.exp(hi[2])) + 1e-6).all()
    assert (p[:, 3] >= lo[3]).all() and (p[:, 3] <= hi[3]).all()
    assert (ref["steps"][..., 4] > 0).all() and (np.diff(ref["steps"][..., 4], axis=-1) > 0).all()      # the clocks move forward
    if name == "every_packet_lost":
        assert (ref["steps"][..., 1] == 0).all() and ref["steps"][..., 2].sum() > 0
    if name == "slow_lossy_shallow":
        assert (p[:, 4] < 40.0).any()          # (starting rates below MIN_RATE are in the batch)
    if name == "fast_deep_short":
        assert (ref["steps"][..., 0] <= 1).any() and (p[:, 2] > 22000).all()      # (intervals of one packet or none)


@pytest.mark.parametrize("delta_scale", [0.025, 0.2, 1.0])
def test_infinite_and_overflowing_rate_actions_run_finite(delta_scale):
    """+-inf and +-1e308 are not NaN: inf * scale is inf, rate * (1 + inf) is inf and rate / (1 + inf) is 0 -- the two clamps
    (ns:275-281) take them to MAX_RATE and MIN_RATE.  The rate column shows exactly that."""
    n, T, seed = 32, 20, 15
    a = extreme_rate_actions(seed, n, T)
    ref = oracle.run_batch(a, seed=seed, delta_scale=delta_scale)
    assert finite(ref)
    rate = ref["steps"][..., 3]
    assert (rate[a > 1e300] == 1000.0).all() and (rate[a < -1e300] == 40.0).all()
    assert (rate >= 40.0).all() and (rate <= 1000.0).all()


def test_delta_scale_reaches_the_rate_and_the_window():
    """delta_scale is an argument of every step of the oracle, not a constant: the first step's rate is rate0 * (1 + a * scale)
    (or / (1 - a * scale)), clamped; the window likewise (int(), then [4, 5000])."""
    n, T, seed = 16, 6, 2
    a = actions(seed, n, T)
    for scale in (0.025, 0.2, 1.0):
        ref = oracle.run_batch(a, seed=seed, delta_scale=scale)
        d = a[:, 0] * scale
        r0 = ref["params"][:, 4]
        want = np.clip(np.where(d >= 0, r0 * (1 + d), r0 / (1 - d)), 40.0, 1000.0)
        assert np.array_equal(ref["steps"][:, 0, 3], want), scale
    o = oracle.OracleEnv(delta_scale=1.0)
    o.rng_philox(seed, 0)
    o.use_cwnd(True)
    o.reset()
    assert o.cwnd() == 25
    o.step([0.0, 1.5])
    assert o.cwnd() == 62            # int(25 * 2.5)
    o.step([0.0, -1e6])
    assert o.cwnd() == 4
    o.step([0.0, 1e6])
    assert o.cwnd() == 5000


# ---------------------------------------------------------------------------------------------------------------- latency noise
# MAX_LATENCY_NOISE off the reference's 1.1.  The golden vectors tie both oracles to the unmodified reference at 1.1 only; at
# 1.0 (every factor exactly 1: event times tie), 2 and 16 (packets overtake hundreds of others) the reference of
# tests/test_noise_domain.py is that two independent restatements agree bit for bit: the C oracle here against the Python
# oracle's heapq loop, on the Mersenne-Twister stream; the sorting models against the same Python oracle in
# tests/test_noise_formulation.py (the links that tie at 1.0 come from there).
from oracle.pcc_oracle_py import PyOracleEnv      # noqa: E402
from test_noise_formulation import TIE_LINKS_1, TIE_LINKS_2, equal_time_pairs      # noqa: E402


def c_against_python(seed, T, noise, S=1, fixed=None, cwnd=False, scale=1.0):
    """One env of each oracle on random.Random(seed)'s stream after the constructor's 4 + S discarded draws: every step row,
    observation, heap length and draw count.  Returns the equal-time pairs of the Python heap, summed over the steps' starts."""
    k = 4 + S
    c = oracle.OracleEnv(S)
    c.rng_mt(seed, skip=k)
    c.use_latency_noise(True, noise)
    p = PyOracleEnv(seed=seed, n_senders=S, fixed=fixed, ctor_draws=k, use_cwnd=cwnd, latency_noise=noise)
    if fixed is not None:
        c.set_params(fixed[0], fixed[1], fixed[2], fixed[3], list(fixed[4:4 + S]))
    if cwnd:
        c.use_cwnd(True)
    assert np.array_equal(np.asarray(c.reset()), np.asarray(p.reset()))
    a = np.random.RandomState(seed).uniform(-1, 1.5, (T, S, 2)) * scale
    ties = 0
    for t in range(T):
        ties += equal_time_pairs(p.heap)
        act = a[t] if cwnd else (a[t, :, 0] if S > 1 else a[t, 0, 0])
        oc, _, dc, _ = c.step(act)
        op, _, dp, _ = p.step(act)
        assert np.array_equal(c.last_row, np.array(p.last_rows, dtype=np.float64)), (seed, noise, t)
        assert np.array_equal(np.asarray(oc), np.asarray(op)) and dc == dp, (seed, noise, t)
        # a sender's packets under way are the events of its device heap: the oracle's heap holds them and one SEND per sender
        assert c.heap_len == len(p.heap) == sum(c.in_flight(s) for s in range(S)) + S, (seed, noise, t)
        assert [c.in_flight(s) for s in range(S)] == p.in_flight, (seed, noise, t)
        assert c.rng_draws == p.draws, (seed, noise, t)
    return ties


@pytest.mark.parametrize("cwnd", [False, True])
@pytest.mark.parametrize("n_senders", [1, 2])
@pytest.mark.parametrize("noise", [1.0, 2.0, 16.0])
def test_c_oracle_equals_python_oracle_off_the_reference_noise(noise, n_senders, cwnd):
    for seed in (0, 5):
        c_against_python(seed, 30, noise, n_senders, cwnd=cwnd)
    c_against_python(8, 30, noise, n_senders, cwnd=cwnd, scale=8.0)


@pytest.mark.parametrize("cwnd", [False, True])
@pytest.mark.parametrize("fixed", TIE_LINKS_1 + TIE_LINKS_2)
def test_c_oracle_equals_python_oracle_on_links_that_tie_at_noise_one(fixed, cwnd):
    """Zero actions at 1.0 on the dyadic links: the ties are there (counted on the Python heap), and the C oracle's heap orders
    them as heapq orders the reference's tuples -- (time, sender, 'A' < 'S', hop, latency, dropped)."""
    ties = c_against_python(0, 25, 1.0, len(fixed) - 4, fixed=fixed, cwnd=cwnd, scale=0.0)
    assert ties >= 25, ties


class TraceRng(object):
    """random.Random's two methods the Python oracle uses, replaying a trace (what RNG_TRACE is to the C oracle)."""

    def __init__(self, u):
        self.u, self.pos = u, 0

    def random(self):
        self.pos += 1
        return float(self.u[self.pos - 1])

    def uniform(self, a, b):
        return a + (b - a) * self.random()


def zero_laden_trace(n, length, seed):
    """Uniforms of which half are exactly 0 and a quarter exactly 0.5: at MAX_LATENCY_NOISE = 2 the factors 1 and 1.5 keep the
    event times of a dyadic link dyadic, so events tie although the noise is on -- and now the draw an event gets shows in its
    latency, which it does not at 1.0 (every factor is 1 there whichever draw it is)."""
    rs = np.random.RandomState(seed)
    u = rs.random_sample((n, length))
    pick = rs.randint(0, 4, (n, length))
    return np.where(pick < 2, 0.0, np.where(pick == 2, 0.5, u))


@pytest.mark.parametrize("fixed", TIE_LINKS_1 + TIE_LINKS_2)
def test_c_oracle_equals_python_oracle_on_a_trace_whose_noise_draws_tie(fixed):
    S, T = len(fixed) - 4, 20
    trace = zero_laden_trace(1, 60000, 31)[0]
    c = oracle.OracleEnv(S)
    c.rng_trace(trace)
    c.use_latency_noise(True, 2.0)
    c.set_params(fixed[0], fixed[1], fixed[2], fixed[3], list(fixed[4:]))
    p = PyOracleEnv(seed=0, n_senders=S, fixed=fixed, ctor_draws=0, latency_noise=2.0)
    p.rng = TraceRng(trace)
    assert np.array_equal(np.asarray(c.reset()), np.asarray(p.reset()))
    ties = 0
    for t in range(T):
        ties += equal_time_pairs(p.heap)
        act = np.zeros(S) if S > 1 else 0.0
        c.step(act); p.step(act)
        assert np.array_equal(c.last_row, np.array(p.last_rows, dtype=np.float64)), t
        assert c.rng_draws == p.rng.pos < trace.size, t
    assert ties >= 2 * T, ties
