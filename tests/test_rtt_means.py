"""rtt_means (pcc-rl_amd/csrc/pcc_retire_env.h: NpSumWalk, leaf_sum2), the routine that reproduces np.mean's summation tree on the
device, held to numpy itself: the harness kernel of tests/kernels/rtt_means_harness.hip runs rtt_means<8> and rtt_means<16>,
unchanged, on the case table of tests/models/rtt_cases.py -- every length 1..300 and every edge of the tree up to four chunks,
four kinds of values, windows that wrap their ring at every kind of place, cursors just below 2**32 -- and every result is compared
with np.mean of the Python list of samples as int64 views: there is no tolerance anywhere.  The outputs are prefilled with NaN
and the ring's .x with NaN (only .y may be read).

The harness is a separate compilation of the same source: it holds the algorithm to numpy at inputs the simulator rarely or never
produces; it cannot vouch for the machine code of the six product kernels rtt_means is compiled into.  tests/test_rtt_lengths.py
drives those to the same lengths against the oracle.  What the table covers and that its values show the order of summation is
proved on the CPU, in tests/test_rtt_means_cpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import pcc_rl_amd
from pcc_rl_amd import build as pbuild

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"))
import rtt_cases as rc   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIP_ERROR_INVALID_VALUE = 1


@pytest.fixture(scope="module")
def harness():
    lib = pbuild.build_rtt_harness()        # (a tree built the usual way has it: this compiles only when it is missing or stale)
    L = ctypes.CDLL(lib)
    L.pcc_test_rtt_means.restype = ctypes.c_int
    L.pcc_test_rtt_means.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 3
    return L


@pytest.fixture(scope="module")
def rings():
    """the rings on the device, as double2 records (NaN, lat0), uploaded once"""
    out = []
    for ring in rc.table():
        rec = np.full((ring.size, 2), np.nan)
        rec[:, 1] = ring.y
        out.append(torch.as_tensor(rec, device=DEV))
    return out


def run(L, ring_dev, size, frm, n, halves, dl, lanes):
    """-> (mean_all, lat_inc) float64 arrays, NaN where the harness wrote nothing"""
    k = len(n)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a).astype(dt).view(np.int32 if dt == np.uint32 else dt), device=DEV)
    d_frm, d_n, d_h, d_dl = t(frm, np.uint32), t(n, np.uint32), t(halves, np.uint8), t(dl, np.float64)
    mean = torch.full((k,), float("nan"), dtype=torch.float64, device=DEV)
    inc = torch.full((k,), float("nan"), dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    rc_ = L.pcc_test_rtt_means(ring_dev.data_ptr(), size, d_frm.data_ptr(), d_n.data_ptr(), d_h.data_ptr(), d_dl.data_ptr(), k, lanes,
                               mean.data_ptr(), inc.data_ptr(), st)
    assert rc_ == 0, "HIP error %d" % rc_
    torch.cuda.synchronize()
    return mean.cpu().numpy(), inc.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def results(harness, rings):
    """(ring index, lanes, halves, order) -> (src, mean, inc), each combination launched once, on demand"""
    cache = {}

    def get(r, lanes, halves, order):
        key = (r, lanes, halves, order)
        if key not in cache:
            ring = rc.table()[r]
            src, frm, n, dl = rc.ordered(ring, order, lanes)
            mean, inc = run(harness, rings[r], ring.size, frm, n, np.full(len(n), 1 if halves else 0), np.nan_to_num(dl), lanes)
            cache[key] = (src, mean, inc)
        return cache[key]
    return get


def by_case(src, values):
    out = np.full(int(src.max()) + 1, np.nan)
    out[src[src >= 0]] = values[src >= 0]
    return out


@pytest.mark.parametrize("halves", [True, False], ids=["halves", "no_halves"])
@pytest.mark.parametrize("lanes", [8, 16])
def test_rtt_means_equal_numpy_bit_for_bit(results, lanes, halves):
    """mean_all == np.mean(list(s)) and lat_inc == np.mean(second half) - np.mean(first half) as int64 views (exactly 0.0 without
    halves), every case of the table, in the shuffled order: neighbouring groups of a wavefront at different stages of different
    lists, some of them without samples."""
    refs = rc.references()
    n_cases = 0
    for r, ring in enumerate(rc.table()):
        src, mean, inc = results(r, lanes, halves, "shuffled")
        want_mean, want_inc = refs[r]
        got_mean, got_inc = by_case(src, mean), by_case(src, inc)
        bad = np.flatnonzero(bits(got_mean) != bits(want_mean))
        assert bad.size == 0, ("mean_all", ring.kind, ring.size, ring.variant, [(int(ring.n[i]), int(ring.frm[i]), got_mean[i], want_mean[i]) for i in bad[:5]],
                               "lengths that differ: %s" % sorted(set(ring.n[bad].tolist()))[:40])
        want = want_inc if halves else np.zeros(len(ring))
        bad = np.flatnonzero(bits(got_inc) != bits(want))
        assert bad.size == 0, ("lat_inc", ring.kind, ring.size, ring.variant, [(int(ring.n[i]), int(ring.frm[i]), got_inc[i], want[i]) for i in bad[:5]],
                               "lengths that differ: %s" % sorted(set(ring.n[bad].tolist()))[:40])
        n_cases += len(ring)
    assert n_cases > 10000


@pytest.mark.parametrize("halves", [True, False], ids=["halves", "no_halves"])
def test_eight_and_sixteen_lanes_agree(results, halves):
    for r in range(len(rc.table())):
        a, b = results(r, 8, halves, "shuffled"), results(r, 16, halves, "shuffled")
        for k in (1, 2):
            assert np.array_equal(bits(by_case(a[0], a[k])), bits(by_case(b[0], b[k]))), (r, k)


@pytest.mark.parametrize("halves", [True, False], ids=["halves", "no_halves"])
@pytest.mark.parametrize("lanes", [8, 16])
def test_a_group_does_not_depend_on_its_neighbours(results, lanes, halves):
    """The same case gives the same bits shuffled among other lists, sorted by length (a wavefront of equal lists), and alone in its
    workgroup; and a group without samples leaves its NaN in every ordering."""
    for r, ring in enumerate(rc.table()):
        first = None
        for order in rc.ORDERS:
            src, mean, inc = results(r, lanes, halves, order)
            dead = src < 0
            assert np.isnan(mean[dead]).all() and np.isnan(inc[dead]).all(), (r, order)
            assert not np.isnan(mean[~dead]).any() and not np.isnan(inc[~dead]).any(), (r, order)
            got = (bits(by_case(src, mean)), bits(by_case(src, inc)))
            if first is None:
                first = got
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), (r, order)
        assert np.array_equal(first[0], bits(rc.references()[r][0]))


def test_the_entry_point_refuses_what_it_cannot_run(harness, rings):
    ring = rc.table()[0]
    z = torch.zeros(8, dtype=torch.float64, device=DEV)
    args = lambda size, lanes: (rings[0].data_ptr(), size, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, lanes, z.data_ptr(), z.data_ptr(), None)
    assert harness.pcc_test_rtt_means(*args(ring.size - 1, 8)) == HIP_ERROR_INVALID_VALUE      # not a power of two
    assert harness.pcc_test_rtt_means(*args(ring.size, 4)) == HIP_ERROR_INVALID_VALUE          # lanes: 8 or 16
