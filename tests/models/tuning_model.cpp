// What pcc_set_tuning accepts, key by key, against a list written down from the switch the table in pcc_sim.hip replaced:
// each key at the ends of its range, just outside both, and at NaN -- and what is stored where the value is rounded, clamped or
// saturated.  Runs without a device: it links the host code of pcc_sim.hip (built with the address and undefined-behaviour
// sanitizers by tests/test_tuning_model.py) and calls only pcc::tuning_value, the pure part of pcc_set_tuning.
#include <cmath>
#include <cstdio>

#include "pcc_sim.h"

namespace pcc {
int tuning_value(int key, double value, double *stored);   // pcc_sim.hip
}

namespace {
const double kNone = -1.0;   // (no stored value to compare)
int bad = 0;

void expect(int key, double value, int code, double stored = kNone) {
    double got = kNone;
    const int rc = pcc::tuning_value(key, value, &got);
    const bool wrong_code = rc != code, wrong_value = rc == PCC_OK && stored != kNone && got != stored;
    const bool silent = rc != PCC_OK && pcc_last_error()[0] == '\0';
    if (wrong_code || wrong_value || silent) {
        printf("key %d value %.17g: code %d (expected %d), stored %.17g (expected %.17g), message \"%s\"\n", key, value, rc, code, got, stored,
               pcc_last_error());
        bad++;
    }
}

// a key whose switch case was `if (!(value >= lo && value <= hi)) return PCC_EINVAL`
void ranged(int key, double lo, double hi) {
    expect(key, lo, PCC_OK, lo);
    expect(key, nextafter(lo, -INFINITY), PCC_EINVAL);
    expect(key, NAN, PCC_EINVAL);
    if (hi == INFINITY) return;
    expect(key, hi, PCC_OK, hi);
    expect(key, nextafter(hi, INFINITY), PCC_EINVAL);
}

// ... that stored whatever it was given (as it is, as a flag, or saturated): never refused, NaN included
void unchecked(int key) {
    const double values[] = {-1e300, -1.0, 0.0, 1.0, 1e300, NAN};
    for (double v : values) expect(key, v, PCC_OK);
}

// ... that accepted the listed values only
void one_of(int key, int n_ok, const double *ok, int n_no, const double *no) {
    for (int i = 0; i < n_ok; i++) expect(key, ok[i], PCC_OK, ok[i]);
    for (int i = 0; i < n_no; i++) expect(key, no[i], PCC_EINVAL);
    expect(key, NAN, PCC_EINVAL);
}
}  // namespace

int main() {
    // ROUND_PACKETS, TAKEOVER_LANES, SEND_ENVS_PER_WAVE: the switch tested `value < lo || value > hi`, which let NaN through to a
    // float-to-integer cast that is undefined (and, at 0 envs per item, to a division by zero in the grid formula).  NaN is in
    // no range: the table refuses it like every other ranged key.  Everything else below is the switch's answer.
    ranged(PCC_TUNE_ROUND_PACKETS, 4, 1048576);
    expect(PCC_TUNE_ROUND_PACKETS, 5, PCC_OK, 8);        // (a multiple of 4)
    expect(PCC_TUNE_ROUND_PACKETS, 257.9, PCC_OK, 260);
    ranged(PCC_TUNE_TAKEOVER_LANES, 0, 64);
    ranged(PCC_TUNE_SEND_ENVS_PER_WAVE, 1, 64);
    expect(PCC_TUNE_SEND_ENVS_PER_WAVE, 1.5, PCC_OK, 1);   // (truncated)
    unchecked(PCC_TUNE_HEAVY_PREDICT);
    expect(PCC_TUNE_HEAVY_PREDICT, 480.5, PCC_OK, 480.5);
    ranged(PCC_TUNE_SEND_WAVES, 1, 32);
    unchecked(PCC_TUNE_TEAM_PREDICT);
    ranged(PCC_TUNE_HEAVY_ITEM_PACKETS, 0, 1e9);
    expect(PCC_TUNE_HEAVY_ITEM_PACKETS, 0.1, PCC_OK, (double)0.1f);   // (a float)
    ranged(PCC_TUNE_RETIRE_WIDE_PREDICT, 0, INFINITY);
    expect(PCC_TUNE_RETIRE_WIDE_PREDICT, 1e300, PCC_OK, 1e9);   // (the 1e9 clamp)
    expect(PCC_TUNE_RETIRE_WIDE_PREDICT, INFINITY, PCC_OK, 1e9);
    ranged(PCC_TUNE_LIST_MIN_ENVS, 0, 4e9);
    unchecked(PCC_TUNE_RETIRE_SORTED);
    expect(PCC_TUNE_RETIRE_SORTED, 7, PCC_OK, 1);
    expect(PCC_TUNE_RETIRE_SORTED, 0, PCC_OK, 0);
    unchecked(PCC_TUNE_LIGHT_SNAKE);
    unchecked(PCC_TUNE_WAVE_OLDEST_FIRST);
    ranged(PCC_TUNE_PRIO_LEVEL, 0, 3);
    for (int key : {PCC_TUNE_PRIO_LIGHT_ITEMS, PCC_TUNE_PRIO_WAVE_ITEMS}) {
        unchecked(key);
        expect(key, 3.7, PCC_OK, 3);
        expect(key, -3, PCC_OK, 0);
        expect(key, nextafter(4e9, 0), PCC_OK, 3999999999.0);
        expect(key, 4e9, PCC_OK, 4294967295.0);   // (the 4e9 saturation)
        expect(key, 1e300, PCC_OK, 4294967295.0);
    }
    unchecked(PCC_TUNE_PRIO_TEAM);
    ranged(PCC_TUNE_RETIRE_GRID_FRAC, 0, 1);
    expect(PCC_TUNE_RETIRE_GRID_FRAC, 0.125, PCC_OK, 0.125);
    {
        const double ok[] = {1, 8}, no[] = {0, 2, 4, 7.5, 9, nextafter(1.0, 0), nextafter(8.0, 9)};
        one_of(PCC_TUNE_PARTS, 2, ok, 7, no);
    }
    ranged(PCC_TUNE_LIGHT_HALF_PREDICT, 0, INFINITY);
    expect(PCC_TUNE_LIGHT_HALF_PREDICT, 2e9, PCC_OK, 1e9);
    unchecked(PCC_TUNE_FUSED);   // (what it refuses depends on the device: pcc_set_tuning asks the handle)
    {
        const double ok[] = {0, 2}, no[] = {1, -1, 3, nextafter(2.0, 3)};
        one_of(PCC_TUNE_FUSED_ACQUIRE, 2, ok, 4, no);
    }
    ranged(PCC_TUNE_FUSED_LIGHT_WGS, 1, 4096);
    ranged(PCC_TUNE_FUSED_MAX_NAPS, 1, 1024);
    ranged(PCC_TUNE_FUSED_PARTIAL_NAPS, 0, 1e6);
    unchecked(PCC_TUNE_FUSED_DEBUG);
    expect(PCC_TUNE_FUSED_DEBUG, 5, PCC_OK, 5);
    ranged(PCC_TUNE_FUSED_LIGHT_FRONT, 0, 4096);
    {
        const double ok[] = {0, 1, 2}, no[] = {0.5, -1, 3, nextafter(0.0, -1), nextafter(2.0, 3)};
        one_of(PCC_TUNE_NOISE_SORTED, 3, ok, 5, no);
    }
    ranged(PCC_TUNE_LIGHT_FRONT, 0, 65536);
    {
        const double ok[] = {0, 1}, no[] = {0.5, -1, 2, nextafter(1.0, 2)};
        one_of(PCC_TUNE_ROLLOUT_EPILOGUE, 2, ok, 4, no);
    }
    // retired keys: 20 and 21 as in the switch; 23 and 34 (any value / 0..65536 there) now like them
    for (int key : {PCC_TUNE_SPLIT_STREAMS, PCC_TUNE_LIGHT_FRONT_WGS, PCC_TUNE_RESTART_FORK, PCC_TUNE_LIGHT_WGS}) {
        const double ok[] = {0}, no[] = {1, -1, 32, nextafter(0.0, 1), nextafter(0.0, -1)};
        one_of(key, 1, ok, 5, no);
    }
    // keys of earlier builds and numbers that never were keys
    for (int key : {-1, 0, 1, 6, 7, 37, 1000}) expect(key, 0, PCC_EINVAL);
    if (bad) printf("%d mismatches\n", bad);
    else puts("tuning model: every key as listed");
    return bad ? 1 : 0;
}
