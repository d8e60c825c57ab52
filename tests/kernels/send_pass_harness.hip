// send_pass_harness.hip -- TEST ONLY (tests/test_send_pass_device.py), never part of libpcc_sim.so: the wave passes of the send half
// (pcc_wave_pass.h, included unchanged) on states the test chooses, one monitor interval per case.
//   variant 0: heavy_mi<TRACE, 1, false>   one wavefront per case, four cases per 256-thread workgroup (as the product's kernels place them)
//   variant 1: heavy_mi<TRACE, 1, true>    the same, the records of a closed-form pass leaving through the wavefront's LDS stage slots
//   variant 2: heavy_mi<TRACE, 4, true>    one workgroup per case: a team pass, TeamX in LDS
//   two senders: heavy_mi2<TRACE, false> and heavy_mi2<TRACE, true>, placed like variants 0 and 1
// TRACE = true: the loss decisions come from the case's row of uniforms (trace + trace_off, trace_stride of them); TRACE = false:
// from Philox with the case's thr / always / episode / mi / gid and the launch's key.
// A separate compilation of the same source: it holds the source-level passes to the plain recurrence (tests/models/send_pass_cases.py)
// at states the simulator rarely or never produces; the product's machine code is held by the simulator's parity tests.
//
// All rings of a launch live in one ARENA of `arena_records` double2 records; a sender's ring is (offset in records, cap): cap accepted
// slots followed by 2 cap dropped slots, as the product lays them out.  Every case is validated ON THE DEVICE before anything of it
// touches memory (case_ok / case2_ok below); a case that fails keeps the test's prefill in its outputs: no mistake in a table can
// make the kernel write outside the arena (ring offsets are masked with cap - 1 / 2 cap - 1 inside a validated ring), read outside
// the trace, or run long (a pass commits at least one packet, and the packets of an interval are bounded by max_packets).
// -DPCC_PROFILE=1 (libpcc_send_harness_prof.so): the passes count themselves into `stats`, 16 + PCC_PATH_SLOTS counters laid out as
// pcc_debug_pass_stats / pcc_debug_path_stats report them.  The plain build ignores `stats`.
#include <hip/hip_runtime.h>

#include "pcc_wave_pass.h"

namespace {

struct SendCase {   // 136 bytes, the layout of tests/models/send_pass_cases.py: CASE1
    double q, tu, t, dl, lr, maxq, ebw, gap, end;
    uint32_t a, d, sent, thr, always, episode, mi, gid, cap, pad;
    uint64_t ring_off;                 // first record of the ring in the arena
    int64_t trace_off, trace_stride;   // the case's uniforms (TRACE)
};
static_assert(sizeof(SendCase) == 136, "layout shared with the test");

struct SendOut {    // 40 bytes
    double q, tu, t;
    uint32_t a, d, sent, flags;
};
static_assert(sizeof(SendOut) == 40, "layout shared with the test");

struct SendCase2 {  // 176 bytes: CASE2
    double q, tu, t[2], dl, lr, maxq, ebw, gap[2], end;
    uint32_t a[2], d[2], sent[2], thr, always, episode, mi, gid, pad;
    uint32_t cap[2];
    uint64_t ring_off[2];
    int64_t trace_off, trace_stride;
};
static_assert(sizeof(SendCase2) == 176, "layout shared with the test");

struct SendOut2 {   // 64 bytes
    double q, tu, t[2];
    uint32_t a[2], d[2], sent[2], flags, pad;
};
static_assert(sizeof(SendOut2) == 64, "layout shared with the test");

constexpr uint32_t kMaxCap = 1u << 20;           // (cap << 4 and 2 cap << 4 stay far inside 32 bits)
constexpr uint64_t kMaxArena = 1ull << 26;       // records: 1 GB
constexpr uint32_t kMaxPacketCap = 8192;
constexpr int kStatSlots = 16 + PCC_PATH_SLOTS;

__device__ __forceinline__ bool is_finite(double x) { return fabs(x) < __builtin_inf(); }   // (false for NaN)

__device__ __forceinline__ bool ring_ok(uint64_t arena_records, uint64_t off, uint32_t cap) {
    return cap >= 64u && cap <= kMaxCap && (cap & (cap - 1u)) == 0u && off <= arena_records && 3ull * cap <= arena_records - off;
}

template <bool TRACE>
__device__ __forceinline__ bool trace_ok(int64_t trace_len, int64_t off, int64_t stride) {
    return !TRACE || (off >= 0 && stride >= 0 && off <= trace_len && stride <= trace_len - off);
}

// one sender's clock: the interval holds at most max_packets packets, and every t += gap moves the clock up to `end`
__device__ __forceinline__ bool clock_ok(double t, double gap, double end, uint32_t max_packets) {
    if (!(is_finite(t) && is_finite(gap) && is_finite(end) && gap > 0.0 && t >= 0.0)) return false;
    if (!(t + gap > t) || !(fabs(end) + gap > fabs(end))) return false;
    return !(end > t) || (end - t) / gap <= (double)max_packets;
}

__device__ __forceinline__ bool link_ok(double q, double tu, double dl, double lr, double maxq, double ebw) {
    return is_finite(q) && is_finite(tu) && is_finite(dl) && is_finite(lr) && is_finite(maxq) && is_finite(ebw);
}

template <bool TRACE>
__device__ __forceinline__ bool case_ok(const SendCase &C, uint64_t arena_records, int64_t trace_len, uint32_t max_packets) {
    return ring_ok(arena_records, C.ring_off, C.cap) && trace_ok<TRACE>(trace_len, C.trace_off, C.trace_stride) &&
           clock_ok(C.t, C.gap, C.end, max_packets) && link_ok(C.q, C.tu, C.dl, C.lr, C.maxq, C.ebw);
}

template <bool TRACE>
__device__ __forceinline__ bool case2_ok(const SendCase2 &C, uint64_t arena_records, int64_t trace_len, uint32_t max_packets) {
    return ring_ok(arena_records, C.ring_off[0], C.cap[0]) && ring_ok(arena_records, C.ring_off[1], C.cap[1]) &&
           trace_ok<TRACE>(trace_len, C.trace_off, C.trace_stride) && clock_ok(C.t[0], C.gap[0], C.end, max_packets) &&
           clock_ok(C.t[1], C.gap[1], C.end, max_packets) && link_ok(C.q, C.tu, C.dl, C.lr, C.maxq, C.ebw);
}

// what the passes read of Dev: trace_stride, the key, the profile counters
__device__ __forceinline__ Dev dev_of(int64_t trace_stride, uint32_t key0, uint32_t key1, unsigned long long *stats) {
    Dev D = {};
    D.trace_stride = trace_stride;
    D.key0 = key0;
    D.key1 = key1;
    D.pass_stats = stats;
    D.pass_counters = (kProfile && stats != nullptr) ? 1 : 0;
    return D;
}

__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

template <bool TRACE, int W, bool STAGE>
__device__ __forceinline__ void run_case1(const SendCase &C, char *arena, const double *trace, uint32_t key0, uint32_t key1,
                                          unsigned long long *stats, uint32_t lane, uint32_t wv, TeamX *X, double2 *stage, SendOut *out) {
    const Dev D = dev_of(C.trace_stride, key0, key1, stats);
    SendState st;
    st.q = C.q; st.tu = C.tu; st.t = C.t;
    st.a = C.a; st.d = C.d; st.sent = C.sent; st.flags = 0;
    st.prof_closed = 0; st.prof_other = 0;
    heavy_mi<TRACE, W, STAGE>(D, lane, wv, X, C.dl, C.lr, C.thr, C.always != 0u, C.maxq, C.ebw, C.gap, C.end, C.episode, C.mi, C.gid,
                              TRACE ? trace + C.trace_off : nullptr, arena + (C.ring_off << 4), C.cap, st, stage);
    if (lane == 0 && (W == 1 || wv == 0u)) {
        out->q = st.q; out->tu = st.tu; out->t = st.t;
        out->a = st.a; out->d = st.d; out->sent = st.sent; out->flags = st.flags;
    }
}

// variants 0 and 1: four cases per workgroup, one per wavefront
template <bool TRACE, bool STAGE>
__global__ __launch_bounds__(256) void send1_wave_kernel(const SendCase *cases, int64_t n_cases, char *arena, uint64_t arena_records,
                                                         const double *trace, int64_t trace_len, uint32_t max_packets, uint32_t key0,
                                                         uint32_t key1, unsigned long long *stats, SendOut *out) {
    __shared__ double2 stage[4][4 * kWave + 1];
    const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t c = uniform_i64((int64_t)blockIdx.x * 4 + wv);
    if (c >= n_cases) return;
    const SendCase C = cases[c];
    if (!case_ok<TRACE>(C, arena_records, trace_len, max_packets)) return;   // (wave-uniform)
    run_case1<TRACE, 1, STAGE>(C, arena, trace, key0, key1, stats, lane, 0u, nullptr, STAGE ? stage[wv] : nullptr, out + c);
}

// variant 2: one case per workgroup, its four wavefronts a team
template <bool TRACE>
__global__ __launch_bounds__(256) void send1_team_kernel(const SendCase *cases, int64_t n_cases, char *arena, uint64_t arena_records,
                                                         const double *trace, int64_t trace_len, uint32_t max_packets, uint32_t key0,
                                                         uint32_t key1, unsigned long long *stats, SendOut *out) {
    __shared__ double2 stage[4][4 * kWave + 1];
    __shared__ TeamX team;
    const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t c = uniform_i64((int64_t)blockIdx.x);
    if (c >= n_cases) return;
    const SendCase C = cases[c];
    if (!case_ok<TRACE>(C, arena_records, trace_len, max_packets)) return;   // (the same for the whole workgroup)
    run_case1<TRACE, 4, true>(C, arena, trace, key0, key1, stats, lane, wv, &team, stage[wv], out + c);
}

template <bool TRACE, bool STAGE>
__global__ __launch_bounds__(256) void send2_wave_kernel(const SendCase2 *cases, int64_t n_cases, char *arena, uint64_t arena_records,
                                                         const double *trace, int64_t trace_len, uint32_t max_packets, uint32_t key0,
                                                         uint32_t key1, unsigned long long *stats, SendOut2 *out) {
    __shared__ double2 stage[4][4 * kWave + 1];
    const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t c = uniform_i64((int64_t)blockIdx.x * 4 + wv);
    if (c >= n_cases) return;
    const SendCase2 C = cases[c];
    if (!case2_ok<TRACE>(C, arena_records, trace_len, max_packets)) return;
    const Dev D = dev_of(C.trace_stride, key0, key1, stats);
    SendState2 st;
    st.q = C.q; st.tu = C.tu; st.flags = 0;
    st.prof_closed = 0; st.prof_other = 0; st.prof_why = 0;
    for (int s = 0; s < 2; s++) { st.t[s] = C.t[s]; st.a[s] = C.a[s]; st.d[s] = C.d[s]; st.sent[s] = C.sent[s]; }
    heavy_mi2<TRACE, STAGE>(D, lane, C.dl, C.lr, C.thr, C.always != 0u, C.maxq, C.ebw, C.gap[0], C.gap[1], C.end, C.episode, C.mi, C.gid,
                            TRACE ? trace + C.trace_off : nullptr, arena + (C.ring_off[0] << 4), arena + (C.ring_off[1] << 4), C.cap[0],
                            C.cap[1], st, STAGE ? stage[wv] : nullptr);
    if (lane == 0) {
        SendOut2 &o = out[c];
        o.q = st.q; o.tu = st.tu; o.flags = st.flags;
        for (int s = 0; s < 2; s++) { o.t[s] = st.t[s]; o.a[s] = st.a[s]; o.d[s] = st.d[s]; o.sent[s] = st.sent[s]; }
    }
}

bool launch_ok(const void *cases, int64_t n_cases, const void *arena, uint64_t arena_records, int trace_mode, const void *trace,
               int64_t trace_len, uint32_t max_packets, const void *out) {
    if (!cases || !arena || !out || n_cases < 0 || n_cases > (1 << 20)) return false;
    if (arena_records == 0 || arena_records > kMaxArena || max_packets == 0 || max_packets > kMaxPacketCap) return false;
    if (trace_mode != 0 && trace_mode != 1) return false;
    if (trace_mode == 1 && (!trace || trace_len <= 0)) return false;
    return true;
}

}  // namespace

// 1 in the -DPCC_PROFILE=1 build (the passes count themselves), 0 in the plain build
extern "C" int pcc_test_send_profile(void) { return kProfile ? 1 : 0; }
// counters of a `stats` block (unsigned 64-bit each): [0, 16) as pcc_debug_pass_stats, [16, 16 + PCC_PATH_SLOTS) the PCC_PATH_* slots
extern "C" int pcc_test_send_stat_slots(void) { return kStatSlots; }
// where in a `stats` block the packets of a path are counted, from the PCC_PATH_* enum this file was compiled with (so that the test
// restates no slot number): which = 0..4 regime A, B with the scan, B without, C, the serial pass of a wavefront; 5..9 the same of a
// team; 10..13 two senders: the token pass, the 256-position sweeps, the 64-lane sweeps, the plain recurrence.  -1: no such path.
extern "C" int pcc_test_send_packet_slot(int which) {
    static const int slots[14] = {PCC_PATH_A_PACKETS, PCC_PATH_B_SCAN_PACKETS, PCC_PATH_B_FREE_PACKETS, PCC_PATH_C_PACKETS, PCC_PATH_SERIAL_PACKETS,
                                  PCC_PATH_TEAM_A_PACKETS, PCC_PATH_TEAM_B_SCAN_PACKETS, PCC_PATH_TEAM_B_FREE_PACKETS, PCC_PATH_TEAM_C_PACKETS,
                                  PCC_PATH_TEAM_SERIAL_PACKETS, PCC_PATH2_TOKEN_PACKETS, PCC_PATH2_SWEEP256_PACKETS, PCC_PATH2_SWEEP64_PACKETS,
                                  PCC_PATH2_PLAIN_PACKETS};
    return which >= 0 && which < 14 ? 16 + slots[which] : -1;
}

// Every pointer but `stream` is device memory.  Returns the HIP error code; hipErrorInvalidValue (and launches nothing) for a null
// pointer, an empty or oversized arena, a packet cap outside 1 .. 8192, an unknown variant / trace mode, or trace mode 1 without a
// trace; n_cases == 0 is hipSuccess without a launch.  The rings of different cases must not overlap.
extern "C" int pcc_test_send1(int variant, int trace_mode, const void *cases, int64_t n_cases, void *arena, uint64_t arena_records,
                              const double *trace, int64_t trace_len, uint32_t max_packets, uint32_t key0, uint32_t key1, void *stats,
                              void *out, void *stream) {
    if (!launch_ok(cases, n_cases, arena, arena_records, trace_mode, trace, trace_len, max_packets, out) || variant < 0 || variant > 2)
        return (int)hipErrorInvalidValue;
    if (n_cases == 0) return (int)hipSuccess;
    const SendCase *cs = (const SendCase *)cases;
    char *ar = (char *)arena;
    unsigned long long *stt = (unsigned long long *)stats;
    SendOut *o = (SendOut *)out;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = variant == 2 ? (unsigned)n_cases : (unsigned)((n_cases + 3) / 4);
#define PCC_SEND1_LAUNCH(K) hipLaunchKernelGGL(K, dim3(blocks), dim3(256), 0, s, cs, n_cases, ar, arena_records, trace, trace_len, max_packets, key0, key1, stt, o)
    if (variant == 0 && trace_mode) PCC_SEND1_LAUNCH((send1_wave_kernel<true, false>));
    else if (variant == 0) PCC_SEND1_LAUNCH((send1_wave_kernel<false, false>));
    else if (variant == 1 && trace_mode) PCC_SEND1_LAUNCH((send1_wave_kernel<true, true>));
    else if (variant == 1) PCC_SEND1_LAUNCH((send1_wave_kernel<false, true>));
    else if (trace_mode) PCC_SEND1_LAUNCH((send1_team_kernel<true>));
    else PCC_SEND1_LAUNCH((send1_team_kernel<false>));
#undef PCC_SEND1_LAUNCH
    return (int)hipGetLastError();
}

// two senders: staged = 0 / 1 for heavy_mi2<TRACE, false> / <TRACE, true>
extern "C" int pcc_test_send2(int staged, int trace_mode, const void *cases, int64_t n_cases, void *arena, uint64_t arena_records,
                              const double *trace, int64_t trace_len, uint32_t max_packets, uint32_t key0, uint32_t key1, void *stats,
                              void *out, void *stream) {
    if (!launch_ok(cases, n_cases, arena, arena_records, trace_mode, trace, trace_len, max_packets, out) || staged < 0 || staged > 1)
        return (int)hipErrorInvalidValue;
    if (n_cases == 0) return (int)hipSuccess;
    const SendCase2 *cs = (const SendCase2 *)cases;
    char *ar = (char *)arena;
    unsigned long long *stt = (unsigned long long *)stats;
    SendOut2 *o = (SendOut2 *)out;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((n_cases + 3) / 4);
#define PCC_SEND2_LAUNCH(K) hipLaunchKernelGGL(K, dim3(blocks), dim3(256), 0, s, cs, n_cases, ar, arena_records, trace, trace_len, max_packets, key0, key1, stt, o)
    if (staged && trace_mode) PCC_SEND2_LAUNCH((send2_wave_kernel<true, true>));
    else if (staged) PCC_SEND2_LAUNCH((send2_wave_kernel<false, true>));
    else if (trace_mode) PCC_SEND2_LAUNCH((send2_wave_kernel<true, false>));
    else PCC_SEND2_LAUNCH((send2_wave_kernel<false, false>));
#undef PCC_SEND2_LAUNCH
    return (int)hipGetLastError();
}
