"""GPU parity of USE_LATENCY_NOISE with MAX_LATENCY_NOISE off the reference's 1.1 -- pcc_set_latency_noise takes [1, 16], and every
other file passes 1.1 -- against the C oracle, bit for bit: np.array_equal on the 19 step columns, the observations and the first
observation, check_flags() clean, unless a case says otherwise.  The route is chosen with set_tuning(noise_sorted=k): 1 = both
instances of the sorting kernels (pcc-rl_amd/csrc/pcc_noise_sorted.hip) and the event loop for what they leave, 2 = the small
instance and the event loop, 0 = the event loop (pcc_retire_env.h: event_engine) for every env.

The reference side is checked by itself on the CPU: off 1.1 no golden vector exists, and the reference is that independent
restatements agree -- tests/test_oracle_settings_cpu.py (C oracle against Python oracle) and tests/test_noise_formulation.py (the
sorting models against the Python oracle, and that the links of section b do tie at 1.0).

  a. values: 1.0 (noise_span == 0: draws consumed, factors exactly 1), 2 and 16 (packets overtake hundreds of others: due events
     pile up, intervals of thousands of SENDs run as sub-intervals)
  b. ties at 1.0: links and actions on which event times are equal
     ... and at 2.0 on a replayed trace full of zero draws, where the draw a tied event takes shows in its latency
  c. which kernel ran an interval is judged from the oracle's counts alone (the asserts of `interval_classes`)
  d. small rings: the hand-over to the event loop and back, PCC_FLAG_RING_OVERFLOW
  e. PCC_FLAG_TRACE_OVERRUN
  f. the domain of pcc_set_latency_noise
Sizes: at most 256 envs and 40 steps, link ranges chosen so that the oracle's longest interval stays near 3 000 SENDs (the event
loop runs an interval event by event on one lane)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import oracle
import pcc_rl_amd
from pcc_rl_amd import native
from test_gpu_parity import DEV, run_gpu
from test_noise_formulation import TIE_LINKS_1, TIE_LINKS_2, tie_actions
from test_oracle_settings_cpu import zero_laden_trace
from test_settings_parity import same_as_oracle, step_against_oracle_envs

pytestmark = pytest.mark.gpu
Env = pcc_rl_amd.BatchedNetworkEnv
ROUTES = [1, 2, 0]

# (lo, hi) of (bandwidth, one-way latency, queue exponent, loss, rate0 / bw) per noise value: an interval lasts half a mean RTT,
# i.e. about (1 + max_noise) / 2 one-way latencies, so the latencies shrink as the noise grows
RANGES = {
    1.0: ((100.0, 0.1, 0.0, 0.0, 0.5), (500.0, 0.6, 5.0, 0.05, 2.0)),
    2.0: ((100.0, 0.05, 0.0, 0.0, 0.3), (500.0, 0.5, 6.0, 0.05, 1.5)),
    16.0: ((100.0, 0.02, 0.0, 0.0, 0.3), (500.0, 0.12, 4.0, 0.05, 1.5)),
}
MAX_INTERVAL = 3600      # SENDs of both senders in the longest interval of any case below ("about 3 000")


def interval_classes(ref, n_senders):
    """Env-intervals by the SENDs of the interval (both senders'), from the oracle alone -- the device has no route counter:
    [fits the first instance, the second instance in one go, sub-intervals].  One sender: <= 128, <= 512, more
    (noise_sorted_kernel<256, 128> and <1024, 512>); two: <= 128, <= 256, more (noise_sorted2_kernel<256, 128> and <512, 256>)."""
    sent = ref["steps"][..., 0] if n_senders == 1 else ref["steps"][..., 0].sum(axis=1)
    b1, b2 = 128, (512 if n_senders == 1 else 256)
    assert sent.max() <= MAX_INTERVAL, sent.max()
    return [int((sent <= b1).sum()), int(((sent > b1) & (sent <= b2)).sum()), int((sent > b2).sum())]


def assert_routes_covered(ref, n_senders, route, what):
    """Section c.  With both instances (route 1) at least 20 env-intervals in each class; with the small instance alone (route 2)
    at least 20 beyond it: the event loop takes those, and the small instance takes the env back."""
    c = interval_classes(ref, n_senders)
    print("env-intervals by SENDs (%s): %s" % (what, c))
    if route == 1:
        assert min(c) >= 20, (what, c)
    if route == 2:
        assert c[1] + c[2] >= 20, (what, c)


@functools.lru_cache(maxsize=None)
def values_case(noise, n_senders, scale):
    n, T, seed = 192, 32, 21
    acts = np.random.RandomState(seed).uniform(-1, 1, (n, T) if n_senders == 1 else (n, T, n_senders)) * scale
    ref = oracle.run_batch(acts, n_senders=n_senders, seed=seed, ranges=RANGES[noise], latency_noise=noise)
    for v in (acts, *[x for x in ref.values() if x is not None]):
        v.setflags(write=False)
    return acts, ref, seed


def run_values(noise, n_senders, route, scale):
    acts, ref, seed = values_case(noise, n_senders, scale)
    what = (noise, n_senders, route, scale)
    assert_routes_covered(ref, n_senders, route, what)
    env = Env(acts.shape[0], device=DEV, seed=seed, n_senders=n_senders, record_steps=True, auto_reset=False, latency_noise=noise)
    env.randomize_link_params(RANGES[noise])
    env.set_tuning(noise_sorted=route)
    obs0 = env.reset().cpu().numpy()
    same_as_oracle(run_gpu(env, acts, acts.shape[1]), ref, obs0, what)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- a. values
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n_senders", [1, 2])
@pytest.mark.parametrize("noise", [1.0, 2.0, 16.0])
def test_noise_values_match_oracle(noise, n_senders, route):
    """Philox, random links, U(-1, 1) actions.  A kernel that read a constant for noise_span, or whose sub-intervals (take_due, the
    K >>= 1 shortening, the block width W = dl / gap - 1) mis-number a draw, differs in the loss and latency columns."""
    run_values(noise, n_senders, route, 1.0)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n_senders", [1, 2])
def test_rates_from_floor_to_ceiling_at_noise_two(n_senders, route):
    """Actions x 8: x 1.2 or / 1.2 a step, the rates run between MIN_RATE and MAX_RATE inside the episode."""
    acts, ref, _ = values_case(2.0, n_senders, 8.0)
    rate = ref["steps"][..., 3]
    assert (rate == 40.0).any() and (rate == 1000.0).any()
    run_values(2.0, n_senders, route, 8.0)


def noise_oracle_envs(n, seed, noise, n_senders=1, ranges=None, cwnd=False):
    out = []
    for i in range(n):
        o = oracle.OracleEnv(n_senders)
        o.rng_philox(seed, i)
        o.use_latency_noise(True, noise)
        if ranges is not None:
            o.set_ranges(*ranges)
        if cwnd:
            o.use_cwnd(True)
        out.append(o)
    return out


@pytest.mark.parametrize("route", ROUTES)
def test_auto_reset_over_an_episode_boundary_at_noise_sixteen(route):
    """Episodes of 12 steps, 30 steps: every env crosses two boundaries; the loose arrays, the draw counters and the interval
    index start over with the episode (each env against its own oracle object)."""
    n, T, seed, noise, max_steps = 96, 30, 22, 16.0, 12
    env = Env(n, device=DEV, seed=seed, record_steps=True, auto_reset=True, max_steps=max_steps, latency_noise=noise)
    env.randomize_link_params(RANGES[noise])
    env.set_tuning(noise_sorted=route)
    oenvs = noise_oracle_envs(n, seed, noise, ranges=RANGES[noise])
    obs0 = env.reset().cpu().numpy()
    assert np.array_equal(obs0, np.stack([o.reset() for o in oenvs]).astype(np.float32))
    acts = np.random.RandomState(seed).uniform(-1, 1, (n, T))
    osteps = np.zeros(n, dtype=int)
    for t in range(T):
        step_against_oracle_envs(env, oenvs, acts[:, t], osteps, max_steps, t)
    env.check_flags()
    env.close()


@pytest.mark.parametrize("n_senders", [1, 2])
@pytest.mark.parametrize("noise", [1.0, 16.0])
def test_window_together_with_noise_off_the_reference_value(noise, n_senders):
    """use_cwnd and latency noise together: the event-loop build whatever the tuning says (one route).  Rate and window actions
    U(-1, 1.5), every env against its own oracle object, the window after every step."""
    n, T, seed = 128, 24, 23
    env = Env(n, device=DEV, seed=seed, n_senders=n_senders, record_steps=True, auto_reset=False, use_cwnd=True, latency_noise=noise)
    env.randomize_link_params(RANGES[noise])
    oenvs = noise_oracle_envs(n, seed, noise, n_senders, RANGES[noise], cwnd=True)
    obs0 = env.reset().cpu().numpy()
    want0 = np.stack([np.asarray(o.reset()).reshape(n_senders, -1) for o in oenvs])
    assert np.array_equal(obs0.reshape(n, n_senders, -1), want0.astype(np.float32))
    acts = np.random.RandomState(seed).uniform(-1, 1.5, (n, T, n_senders, 2))
    osteps = np.zeros(n, dtype=int)
    for t in range(T):
        step_against_oracle_envs(env, oenvs, acts[:, t], osteps, 400, t, cwnd=True)
    env.check_flags()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- b. ties
@functools.lru_cache(maxsize=None)
def ties_case(n_senders):
    """The dyadic links of tests/test_noise_formulation.py, an equal share of the batch each; tie_actions (there): zero for ten
    steps, then +-2 at delta_scale = 0.5 -- the rate doubles or halves, 1 / rate stays a power of two until a clamp -- for the
    first half of every share and U(-1, 1) for the rest.  That these inputs tie is asserted on the CPU, in that file."""
    links = TIE_LINKS_1 if n_senders == 1 else TIE_LINKS_2
    n, T, seed = 192, 30, 24
    params = np.array([links[(i * len(links)) // n] for i in range(n)], dtype=np.float64)
    acts = tie_actions(n, T, n_senders, seed, shares=len(links))
    ref = oracle.run_batch(acts, n_senders=n_senders, seed=seed, params=params, delta_scale=0.5, latency_noise=1.0)
    for v in (acts, params, *[x for x in ref.values() if x is not None]):
        v.setflags(write=False)
    return acts, params, ref, seed


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n_senders", [1, 2])
def test_equal_event_times_at_noise_one_are_ordered_as_the_reference_orders_them(n_senders, route):
    """(time, sender, ACK before SEND, hop, latency, dropped): the device restates that order in the kernels' ev_less / ev_less2
    and the heap's heap_less, in count_lt against count_le where the SENDs before an arrival are counted, and in the choice of
    the event that ends the interval.  At 1.1 a tie has probability zero; here hundreds of events per env share their time, and
    a copy that breaks one the other way hands a SEND's loss draw to an arrival: the lost and latency columns differ."""
    acts, params, ref, seed = ties_case(n_senders)
    S = n_senders
    env = Env(acts.shape[0], device=DEV, seed=seed, n_senders=S, record_steps=True, auto_reset=False, latency_noise=1.0, delta_scale=0.5)
    env.set_link_params(params[:, 0], params[:, 1], params[:, 2], params[:, 3], params[:, 4] if S == 1 else params[:, 4:6])
    env.set_tuning(noise_sorted=route)
    obs0 = env.reset().cpu().numpy()
    same_as_oracle(run_gpu(env, acts, acts.shape[1]), ref, obs0, (S, route))
    env.close()


@functools.lru_cache(maxsize=None)
def tied_draws_case(n_senders):
    """The dyadic links at MAX_LATENCY_NOISE = 2 on a replayed trace of which half the uniforms are 0 and a quarter 0.5
    (zero_laden_trace, tests/test_oracle_settings_cpu.py, where both oracles are compared on it): the factors 1 and 1.5 keep the
    times dyadic, events tie, and the draw an event is given shows in its latency.  Zero actions for ten steps, then tie_actions."""
    links = TIE_LINKS_1 if n_senders == 1 else TIE_LINKS_2
    n, T, seed = 96, 20, 29
    params = np.array([links[(i * len(links)) // n] for i in range(n)], dtype=np.float64)
    acts = tie_actions(n, T, n_senders, seed, shares=len(links))
    trace = zero_laden_trace(n, 60000, seed)
    ref = oracle.run_batch(acts, n_senders=n_senders, rng_mode=oracle.RNG_TRACE, trace=trace, params=params, delta_scale=0.5, latency_noise=2.0)
    return acts, params, trace, ref


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n_senders", [1, 2])
def test_tied_events_take_the_draws_the_reference_gives_them(n_senders, route):
    """At 1.0 the order of tied events decides which draw each takes, but every factor is 1 whichever it is.  Here a SEND and an
    arrival of equal time, or two arrivals of equal time and different latency, get different factors if the device orders them
    otherwise than (time, sender, ACK before SEND, hop, latency, dropped) -- count_lt against count_le, ev_less."""
    acts, params, trace, ref = tied_draws_case(n_senders)
    S = n_senders
    env = Env(acts.shape[0], device=DEV, n_senders=S, record_steps=True, auto_reset=False, latency_noise=2.0, delta_scale=0.5)
    env.set_link_params(params[:, 0], params[:, 1], params[:, 2], params[:, 3], params[:, 4] if S == 1 else params[:, 4:6])
    env.set_loss_trace(trace)
    env.set_tuning(noise_sorted=route)
    obs0 = env.reset().cpu().numpy()
    same_as_oracle(run_gpu(env, acts, acts.shape[1]), ref, obs0, (S, route))
    env.close()


# ---------------------------------------------------------------------------------------------------------------- d. small rings
def ring_links(n, cap, n_senders):
    """Fast links without loss to speak of, the starting rates swept so that (events in flight) + (SENDs of an interval) runs from
    about half the capacity to about twice: at max_noise = 16 a mean RTT is 17 one-way latencies, an interval half of that.  Half
    the batch sits just below the capacity, where an env fits and comes within 64 of it; the latency grows with the capacity, so
    that the rates are the same at both."""
    dl = 0.05 * cap / 256
    q = n // 16
    target = np.concatenate([np.linspace(0.45, 0.8, 3 * q), np.linspace(0.8, 1.05, 8 * q), np.linspace(1.05, 1.3, 2 * q),
                             np.linspace(1.3, 2.2, n - 13 * q)]) * cap          # about 25.5 * rate * dl per sender
    rate0 = np.clip(target / (25.5 * dl), 45.0, 990.0)
    p = np.zeros((n, 4 + n_senders))
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = 4000.0, dl, 64.0, 0.01
    for s in range(n_senders):
        p[:, 4 + s] = rate0 if s == 0 else np.clip(rate0 * 0.8, 45.0, 990.0)
    return p


@functools.lru_cache(maxsize=None)
def ring_case(cap, n_senders):
    """Every env stepped by its own oracle object: the rows, the observations, and per step and sender the packets under way at
    the step's start and end.  A sender's device array holds one event per packet under way (event_engine pushes one per SEND and
    pops it when the sender hears of the packet), which is the oracle's in_flight: its heap_len == sum of in_flight + one pending
    SEND per sender (asserted here and in tests/test_oracle_settings_cpu.py)."""
    n, T, seed, noise, S = 256, 30, 25, 16.0, n_senders
    params = ring_links(n, cap, S)
    acts = np.random.RandomState(seed).uniform(-1, 1, (n, T, S))
    rows, obs = np.zeros((n, S, T, 19)), np.zeros((n, S, T, 30))
    obs0, count = np.zeros((n, S, 30)), np.zeros((n, S, T + 1), dtype=np.int64)
    for i in range(n):
        o = oracle.OracleEnv(S)
        o.rng_philox(seed, i)
        o.use_latency_noise(True, noise)
        o.set_params(params[i, 0], params[i, 1], params[i, 2], params[i, 3], params[i, 4:])
        obs0[i] = np.asarray(o.reset()).reshape(S, -1)
        count[i, :, 0] = [o.in_flight(s) for s in range(S)]
        for t in range(T):
            ob, _, _, _ = o.step(acts[i, t])
            rows[i, :, t], obs[i, :, t] = o.last_row, np.asarray(ob).reshape(S, -1)
            count[i, :, t + 1] = [o.in_flight(s) for s in range(S)]
            assert o.heap_len == count[i, :, t + 1].sum() + S
        o.close()
    sent, acked = rows[..., 0].astype(np.int64), rows[..., 1].astype(np.int64)
    need = count[..., :-1] + sent + 2                     # the sorted kernels' `room` test, whole interval: n_heap + K + 2 < cap
    # the two warm-up intervals of reset() are not in the rows: at most rate0 * 3 dl + 1 SENDs each, nothing in flight before
    warm = 2.0 * (params[:, 4:] * 3.0 * params[:, 1:2] + 1.0) + 2.0
    fits = ((need < cap).all(axis=2) & (acked <= cap).all(axis=2) & (warm < cap)).all(axis=1)
    overflows = (count > cap).any(axis=2).any(axis=1)
    near = fits & ((need >= cap - 64).any(axis=2)).any(axis=1)
    assert sent.sum(axis=1).max() <= MAX_INTERVAL
    out = dict(acts=acts, params=params, rows=rows, obs=obs, obs0=obs0, fits=fits, overflows=overflows, near=near, seed=seed, noise=noise)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("n_senders", [1, 2])
@pytest.mark.parametrize("cap", [256, 1024])
def test_small_rings_hand_over_to_the_event_loop_and_flag_what_does_not_fit(cap, n_senders, route):
    """ring_capacity = noise_cap.  The sorted kernels leave an env to the event loop when n_heap + K + 2 >= noise_cap (the loose
    array, bit 31 of heap_n, heapify_if_loose, and back); the event loop raises PCC_FLAG_RING_OVERFLOW at the push that does not fit
    (it pushes while hn < noise_cap).  From the oracle alone, with count = a sender's packets under way:
      fits       at every step count(start) + SENDs + 2 < cap, acknowledgements <= cap (and the warm-up cannot reach cap):
                 bit-equal, no flag
      overflows  count(end of some step) > cap: a push found the array full -- flagged
      between    the rest: bit-equal if not flagged
    and nothing carries another flag.  At least 16 envs fit, 16 overflow, and 16 of those that fit come within 64 of the capacity
    -- the envs that cross from the sorted kernels to the event loop and back (route 1)."""
    c = ring_case(cap, n_senders)
    n, S, T = c["acts"].shape[0], n_senders, c["acts"].shape[1]
    fits, overflows = c["fits"], c["overflows"]
    print("cap %d, %d senders: %d fit (%d of them near the capacity), %d overflow, %d between"
          % (cap, S, fits.sum(), c["near"].sum(), overflows.sum(), n - fits.sum() - overflows.sum()))
    assert fits.sum() >= 16 and overflows.sum() >= 16 and not (fits & overflows).any()
    assert c["near"].sum() >= 16
    p = c["params"]
    env = Env(n, device=DEV, seed=c["seed"], n_senders=S, record_steps=True, auto_reset=False, latency_noise=c["noise"], ring_capacity=cap)
    env.set_link_params(p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4] if S == 1 else p[:, 4:6])
    env.set_tuning(noise_sorted=route)
    obs0 = env.reset().cpu().numpy().reshape(n, S, -1)
    a = torch.as_tensor(c["acts"] if S == 2 else c["acts"][:, :, 0], dtype=torch.float64, device=DEV)
    rows, obs = [], []
    for t in range(T):
        o, _, _, info = env.step(a[:, t])
        rows.append(info["steps"].clone().reshape(n, S, -1)); obs.append(o.clone().reshape(n, S, -1))
    torch.cuda.synchronize()
    rows, obs = torch.stack(rows, 2).cpu().numpy(), torch.stack(obs, 2).cpu().numpy()
    flags = env.state("flags").cpu().numpy().astype(np.int64)
    env.close()
    assert not (flags & ~native.PCC_FLAG_RING_OVERFLOW).any(), np.unique(flags)
    flagged = (flags & native.PCC_FLAG_RING_OVERFLOW) != 0
    assert not flagged[fits].any(), np.flatnonzero(flagged & fits)[:10]
    assert flagged[overflows].all(), np.flatnonzero(~flagged & overflows)[:10]
    ok = ~flagged
    assert np.array_equal(obs0[ok], c["obs0"][ok].astype(np.float32))
    bad = np.flatnonzero(ok & (rows != c["rows"]).any(axis=(1, 2, 3)))
    assert bad.size == 0, ("unflagged envs that differ from the oracle", bad[:10])
    assert np.array_equal(obs[ok], c["obs"][ok].astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- e. the trace runs out
@functools.lru_cache(maxsize=None)
def trace_case(noise):
    """64 fixed links, one sender; a uniform trace per env; the oracle on the whole trace says how many draws each env's 20 steps
    take (fixed links draw nothing at reset: the count is the episode's).  The device gets the trace cut between the two middle
    counts: long enough for half the batch."""
    n, T, seed = 64, 20, 26
    rs = np.random.RandomState(seed)
    params = np.stack([rs.uniform(100, 300, n), rs.uniform(0.03, 0.09, n), rs.randint(2, 40, n).astype(float), rs.uniform(0, 0.04, n),
                       rs.uniform(60, 400, n)], axis=1)
    acts = rs.uniform(-1, 1, (n, T))
    trace = rs.random_sample((n, 24000))
    draws = np.zeros(n, dtype=np.int64)
    for i in range(n):
        o = oracle.OracleEnv()
        o.rng_trace(trace[i])
        if noise:
            o.use_latency_noise(True, noise)
        o.set_params(*params[i, :4], params[i, 4:])
        o.reset()
        for t in range(T):
            o.step(acts[i, t])
        draws[i] = o.rng_draws
        o.close()
    assert draws.max() < trace.shape[1]
    d = np.sort(draws)
    assert d[n // 2] - d[n // 2 - 1] >= 2
    stride = int(d[n // 2 - 1] + d[n // 2]) // 2          # draws <= stride: the trace is long enough
    ref = oracle.run_batch(acts, rng_mode=oracle.RNG_TRACE, trace=trace, params=params, latency_noise=noise)
    return acts, params, trace[:, :stride].copy(), draws <= stride, ref


@pytest.mark.parametrize("engine", ["plain", "noise_sorted1", "noise_sorted0"])
def test_a_trace_that_is_too_short_is_flagged_and_nothing_else_is(engine):
    """PCC_RNG_TRACE with trace_stride between the draw counts of the two halves of the batch: the envs whose episode needs more
    draws than the trace holds carry exactly PCC_FLAG_TRACE_OVERRUN (the plain engine's send paths; draw_at of the sorted kernels;
    draw() of the event loop) and are not compared; the others carry no flag and equal the oracle on the same trace."""
    noise = None if engine == "plain" else 2.0
    acts, params, trace, enough, ref = trace_case(noise)
    n, T = acts.shape
    assert enough.sum() == n // 2
    env = Env(n, device=DEV, record_steps=True, auto_reset=False, latency_noise=noise)
    env.set_link_params(*[params[:, k] for k in range(5)])
    env.set_loss_trace(trace)
    if noise:
        env.set_tuning(noise_sorted=int(engine[-1]))
    obs0 = env.reset().cpu().numpy()
    a = torch.as_tensor(acts, dtype=torch.float64, device=DEV)
    rows, obs = [], []
    for t in range(T):
        o, _, _, info = env.step(a[:, t])
        rows.append(info["steps"].clone()); obs.append(o.clone())
    torch.cuda.synchronize()
    rows, obs = torch.stack(rows, 1).cpu().numpy(), torch.stack(obs, 1).cpu().numpy()
    flags = env.state("flags").cpu().numpy().astype(np.int64)
    env.close()
    assert np.array_equal(flags, np.where(enough, 0, native.PCC_FLAG_TRACE_OVERRUN)), (flags, enough)
    assert np.array_equal(obs0[enough], ref["obs0"][enough].astype(np.float32))
    assert np.array_equal(rows[enough], ref["steps"][enough])
    assert np.array_equal(obs[enough], ref["obs"][enough].astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- f. the domain
def test_max_noise_outside_its_domain_is_refused_and_the_ends_are_accepted():
    """pcc_set_latency_noise(h, 1, x) takes x in [1, 16]: NaN, the doubles next to 1 and 16 on the outside, +-inf and -1 are
    PCC_EINVAL and leave the handle as it was -- a following episode equals the oracle at the value it had (2.0, so that "as it
    was" is neither the reference's 1.1 nor off).  1.0 and 16.0 themselves are accepted, and take effect."""
    n, T, seed = 128, 8, 27
    acts = np.random.RandomState(seed).uniform(-1, 1, (n, T))
    for value in (2.0, 1.0, 16.0):
        env = Env(n, device=DEV, seed=seed, record_steps=True, auto_reset=False, latency_noise=2.0)
        env.randomize_link_params(RANGES[16.0])
        if value == 2.0:
            for bad in (float("nan"), np.nextafter(1.0, 0.0), np.nextafter(16.0, 17.0), float("inf"), float("-inf"), -1.0):
                rc = env._L.pcc_set_latency_noise(env._h, 1, ctypes.c_double(bad))
                assert rc == -1, bad      # PCC_EINVAL
                with pytest.raises(pcc_rl_amd.PccError) as e:
                    native.check(env._L.pcc_set_latency_noise(env._h, 1, ctypes.c_double(bad)))
                assert e.value.code == -1 and "max_noise" in str(e.value), str(e.value)
        else:
            assert env._L.pcc_set_latency_noise(env._h, 1, ctypes.c_double(value)) == 0
        obs0 = env.reset().cpu().numpy()
        ref = oracle.run_batch(acts, seed=seed, ranges=RANGES[16.0], latency_noise=value)
        same_as_oracle(run_gpu(env, acts, T), ref, obs0, value)
        env.close()
    assert not np.array_equal(oracle.run_batch(acts, seed=seed, ranges=RANGES[16.0], latency_noise=1.1, want_obs=False)["steps"],
                              oracle.run_batch(acts, seed=seed, ranges=RANGES[16.0], latency_noise=2.0, want_obs=False)["steps"])


def test_latency_noise_of_one_is_on_and_of_zero_is_off():
    """BatchedNetworkEnv tests its latency_noise argument for truth: 1.0 switches the option on (every factor is 1, but the draws
    are taken: two per SEND and one per arrival, so the loss draws are other draws than without the option), 0.0 and None mean off."""
    n, T, seed = 128, 12, 28
    ranges = ((100.0, 0.05, 0.0, 0.05, 0.3), (500.0, 0.3, 5.0, 0.2, 1.5))      # lossy: the loss column shows which draws were taken
    acts = np.random.RandomState(seed).uniform(-1, 1, (n, T))
    on = oracle.run_batch(acts, seed=seed, ranges=ranges, latency_noise=1.0)
    off = oracle.run_batch(acts, seed=seed, ranges=ranges)
    assert not np.array_equal(on["steps"][..., 2], off["steps"][..., 2])
    for arg, ref in ((1.0, on), (0.0, off), (None, off)):
        env = Env(n, device=DEV, seed=seed, record_steps=True, auto_reset=False, latency_noise=arg)
        assert env.latency_noise == (1.0 if arg else None)
        env.randomize_link_params(ranges)
        obs0 = env.reset().cpu().numpy()
        same_as_oracle(run_gpu(env, acts, T), ref, obs0, arg)
        env.close()
