// retire_search_harness.hip -- TEST ONLY (tests/test_retire_search.py), never part of libpcc_sim.so: the boundary searches and the
// near-group repairs of pcc_retire_env.h -- search_many<4, G>, search_boundary<G>, fix_drop_boundary_g<G>, drop_hop1_candidate_g<G>,
// G = 8 and 16 -- unchanged, on inputs the test chooses.  One group of G lanes per case, the group formed as retire_kernel forms it,
// workgroups of kWalkMaxBlock, different cases side by side in a wavefront: a group whose four predicted windows hold their
// boundaries returns from search_many while its neighbours descend, a group with a short near window partitions it by ballot while
// its neighbour's lead lane walks a long one -- the divergence the product calls them under.  EVERY lane of a group writes what it
// got (the repairs promise the same values on every lane; the callers of search_many read bnd[] on all lanes), `stat` is nullptr.
// A separate compilation of the same source: it holds the algorithm to a linear scan (tests/models/boundary_cases.py), not the
// product's machine code (the simulator's parity tests hold that to the oracle).
//
// All rings of a launch live in one ARENA of `arena_records` double2 records (t1, lat); a ring is (offset in records, mask) and a
// case whose ring does not lie inside the arena, whose mask + 1 is no power of two or whose cursors are out of order is skipped on
// the device (its outputs keep the test's prefill): no index the test gets wrong reaches memory outside the arena.
#include <hip/hip_runtime.h>

#include "pcc_retire_env.h"

namespace {

template <int G>
__device__ __forceinline__ Group form_group(int64_t &c) {
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    Group g;
    g.lane = tid & (uint32_t)(G - 1);
    g.shift = lane & ~(uint32_t)(G - 1);
    c = (int64_t)blockIdx.x * (kWalkMaxBlock / G) + tid / (uint32_t)G;
    return g;
}

// a ring of mask + 1 records at record `off` of the arena, holding the cursor range [lo, hi)
__device__ __forceinline__ bool ring_ok(uint64_t arena_records, uint32_t off, uint32_t mask, uint32_t lo, uint32_t hi) {
    const uint64_t size = (uint64_t)mask + 1u;
    return (size & mask) == 0 && (uint64_t)off + size <= arena_records && lo <= hi && (uint64_t)(hi - lo) <= size;
}

// per search (4 per case, [c * 4 + k]): off, mask, lo0, hi0, add, hint; per case: end.  Outputs [(c * G + lane) * 4 + k].
template <int G>
__global__ __launch_bounds__(kWalkMaxBlock) void search_many_harness_kernel(const double2 *arena, uint64_t arena_records, const uint32_t *off,
                                                                            const uint32_t *mask, const uint32_t *lo0, const uint32_t *hi0,
                                                                            const double *add, const uint32_t *hint, const double *end,
                                                                            int64_t n_cases, uint32_t *out_b, uint8_t *out_clean, double *out_t,
                                                                            double *out_lat) {
    int64_t c;
    const Group g = form_group<G>(c);
    if (c >= n_cases) return;
    bool ok = true;
    for (int k = 0; k < 4; k++) ok = ok && ring_ok(arena_records, off[c * 4 + k], mask[c * 4 + k], lo0[c * 4 + k], hi0[c * 4 + k]);
    if (!ok) return;   // (group-uniform)
    const double2 *const rings[4] = {arena + off[c * 4 + 0], arena + off[c * 4 + 1], arena + off[c * 4 + 2], arena + off[c * 4 + 3]};
    const uint32_t masks[4] = {mask[c * 4 + 0], mask[c * 4 + 1], mask[c * 4 + 2], mask[c * 4 + 3]};
    const uint32_t los[4] = {lo0[c * 4 + 0], lo0[c * 4 + 1], lo0[c * 4 + 2], lo0[c * 4 + 3]};
    const uint32_t his[4] = {hi0[c * 4 + 0], hi0[c * 4 + 1], hi0[c * 4 + 2], hi0[c * 4 + 3]};
    const double adds[4] = {add[c * 4 + 0], add[c * 4 + 1], add[c * 4 + 2], add[c * 4 + 3]};
    const uint32_t hints[4] = {hint[c * 4 + 0], hint[c * 4 + 1], hint[c * 4 + 2], hint[c * 4 + 3]};
    Bound bnd[4];
    for (int k = 0; k < 4; k++) { bnd[k].b = 0xFFFFFFFFu; bnd[k].clean = false; bnd[k].t = 0.0; bnd[k].lat = 0.0; }
    search_many<4, G>(g, rings, masks, los, his, adds, end[c], hints, bnd, nullptr);
    const int64_t o = (c * G + g.lane) * 4;
    for (int k = 0; k < 4; k++) {
        out_b[o + k] = bnd[k].b;
        out_clean[o + k] = bnd[k].clean ? 1 : 0;
        out_t[o + k] = bnd[k].t;
        out_lat[o + k] = bnd[k].lat;
    }
}

// per case: off, mask, lo, hi, add, end.  Output [c * G + lane].
template <int G>
__global__ __launch_bounds__(kWalkMaxBlock) void search_boundary_harness_kernel(const double2 *arena, uint64_t arena_records, const uint32_t *off,
                                                                                const uint32_t *mask, const uint32_t *lo, const uint32_t *hi,
                                                                                const double *add, const double *end, int64_t n_cases,
                                                                                uint32_t *out_idx) {
    int64_t c;
    const Group g = form_group<G>(c);
    if (c >= n_cases) return;
    if (!ring_ok(arena_records, off[c], mask[c], lo[c], hi[c])) return;
    out_idx[c * G + g.lane] = search_boundary<G>(g, arena + off[c], mask[c], lo[c], hi[c], add[c], end[c]);
}

// per case: off, mask (a ring region of its own: the routine rewrites it), h, tail, b, dl, end.  Outputs [c * G + lane].
template <int G>
__global__ __launch_bounds__(kWalkMaxBlock) void fix_drop_harness_kernel(double2 *arena, uint64_t arena_records, const uint32_t *off,
                                                                         const uint32_t *mask, const uint32_t *h, const uint32_t *tail,
                                                                         const uint32_t *b, const double *dl, const double *end, int64_t n_cases,
                                                                         uint32_t *out_p, uint32_t *out_idx, double *out_t, double *out_lat) {
    int64_t c;
    const Group g = form_group<G>(c);
    if (c >= n_cases) return;
    if (!ring_ok(arena_records, off[c], mask[c], h[c], tail[c]) || b[c] < h[c] || b[c] > tail[c]) return;
    const DropFix fx = fix_drop_boundary_g<G>(g.lane, g.shift, arena + off[c], mask[c], h[c], tail[c], b[c], dl[c], end[c]);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // (as the caller does before anybody reads the ring again)
    const int64_t o = c * G + g.lane;
    out_p[o] = fx.p;
    out_idx[o] = fx.cand_idx;
    out_t[o] = fx.cand_t;
    out_lat[o] = fx.cand_lat;
}

// per case: off, mask, h, tail, c (the transition of `t1 < end`), end.  Outputs [c * G + lane].
template <int G>
__global__ __launch_bounds__(kWalkMaxBlock) void drop_hop1_harness_kernel(const double2 *arena, uint64_t arena_records, const uint32_t *off,
                                                                          const uint32_t *mask, const uint32_t *h, const uint32_t *tail,
                                                                          const uint32_t *cc, const double *end, int64_t n_cases, double *out_t,
                                                                          double *out_lat) {
    int64_t c;
    const Group g = form_group<G>(c);
    if (c >= n_cases) return;
    if (!ring_ok(arena_records, off[c], mask[c], h[c], tail[c]) || cc[c] < h[c] || cc[c] > tail[c]) return;
    const Cand cd = drop_hop1_candidate_g<G>(g.lane, g.shift, arena + off[c], mask[c], h[c], tail[c], cc[c], end[c]);
    const int64_t o = c * G + g.lane;
    out_t[o] = cd.t;
    out_lat[o] = cd.lat;
}

// the launch shape of all four entries: 0 blocks for arguments that are refused
unsigned blocks_for(const void *arena, uint64_t arena_records, int64_t n_cases, int lanes) {
    if (!arena || arena_records == 0 || arena_records > (1ull << 28) || (lanes != 8 && lanes != 16) || n_cases <= 0) return 0;
    const int64_t per_block = kWalkMaxBlock / lanes;
    const int64_t blocks = (n_cases + per_block - 1) / per_block;
    return blocks > 0x7FFFFFFF ? 0u : (unsigned)blocks;
}

}  // namespace

// Every array is device memory; every entry returns the HIP error code, hipErrorInvalidValue (and launches nothing) for a null
// pointer, an empty or oversized arena, n_cases < 0 or lanes other than 8 and 16; n_cases == 0 is hipSuccess without a launch.
extern "C" int pcc_test_search_many(const void *arena, uint64_t arena_records, const uint32_t *off, const uint32_t *mask, const uint32_t *lo0,
                                    const uint32_t *hi0, const double *add, const uint32_t *hint, const double *end, int64_t n_cases, int lanes,
                                    uint32_t *out_b, uint8_t *out_clean, double *out_t, double *out_lat, void *stream) {
    if (!off || !mask || !lo0 || !hi0 || !add || !hint || !end || !out_b || !out_clean || !out_t || !out_lat) return (int)hipErrorInvalidValue;
    if (arena && arena_records && arena_records <= (1ull << 28) && (lanes == 8 || lanes == 16) && n_cases == 0) return (int)hipSuccess;
    const unsigned blocks = blocks_for(arena, arena_records, n_cases, lanes);
    if (!blocks) return (int)hipErrorInvalidValue;
    const double2 *a = (const double2 *)arena;
    if (lanes == 8)
        hipLaunchKernelGGL((search_many_harness_kernel<8>), dim3(blocks), dim3(kWalkMaxBlock), 0, (hipStream_t)stream, a, arena_records, off, mask,
                           lo0, hi0, add, hint, end, n_cases, out_b, out_clean, out_t, out_lat);
    else
        hipLaunchKernelGGL((search_many_harness_kernel<16>), dim3(blocks), dim3(kWalkMaxBlock), 0, (hipStream_t)stream, a, arena_records, off, mask,
                           lo0, hi0, add, hint, end, n_cases, out_b, out_clean, out_t, out_lat);
    return (int)hipGetLastError();
}

extern "C" int pcc_test_search_boundary(const void *arena, uint64_t arena_records, const uint32_t *off, const uint32_t *mask, const uint32_t *lo,
                                        const uint32_t *hi, const double *add, const double *end, int64_t n_cases, int lanes, uint32_t *out_idx,
                                        void *stream) {
    if (!off || !mask || !lo || !hi || !add || !end || !out_idx) return (int)hipErrorInvalidValue;
    if (arena && arena_records && arena_records <= (1ull << 28) && (lanes == 8 || lanes == 16) && n_cases == 0) return (int)hipSuccess;
    const unsigned blocks = blocks_for(arena, arena_records, n_cases, lanes);
    if (!blocks) return (int)hipErrorInvalidValue;
    const double2 *a = (const double2 *)arena;
    if (lanes == 8)
        hipLaunchKernelGGL((search_boundary_harness_kernel<8>), dim3(blocks), dim3(kWalkMaxBlock), 0, (hipStream_t)stream, a, arena_records, off,
                           mask, lo, hi, add, end, n_cases, out_idx);
    else
        hipLaunchKernelGGL((search_boundary_harness_kernel<16>), dim3(blocks), dim3(kWalkMaxBlock), 0, (hipStream_t)stream, a, arena_records, off,
                           mask, lo, hi, add, end, n_cases, out_idx);
    return (int)hipGetLastError();
}

// (the regions of different cases must not overlap: the routine rewrites its near window)
extern "C" int pcc_test_fix_drop_boundary(void *arena, uint64_t arena_records, const uint32_t *off, const uint32_t *mask, const uint32_t *h,
                                          const uint32_t *tail, const uint32_t *b, const double *dl, const double *end, int64_t n_cases, int lanes,
                                          uint32_t *out_p, uint32_t *out_idx, double *out_t, double *out_lat, void *stream) {
    if (!off || !mask || !h || !tail || !b || !dl || !end || !out_p || !out_idx || !out_t || !out_lat) return (int)hipErrorInvalidValue;
    if (arena && arena_records && arena_records <= (1ull << 28) && (lanes == 8 || lanes == 16) && n_cases == 0) return (int)hipSuccess;
    const unsigned blocks = blocks_for(arena, arena_records, n_cases, lanes);
    if (!blocks) return (int)hipErrorInvalidValue;
    double2 *a = (double2 *)arena;
    if (lanes == 8)
        hipLaunchKernelGGL((fix_drop_harness_kernel<8>), dim3(blocks), dim3(kWalkMaxBlock), 0, (hipStream_t)stream, a, arena_records, off, mask, h,
                           tail, b, dl, end, n_cases, out_p, out_idx, out_t, out_lat);
    else
        hipLaunchKernelGGL((fix_drop_harness_kernel<16>), dim3(blocks), dim3(kWalkMaxBlock), 0, (hipStream_t)stream, a, arena_records, off, mask, h,
                           tail, b, dl, end, n_cases, out_p, out_idx, out_t, out_lat);
    return (int)hipGetLastError();
}

extern "C" int pcc_test_drop_hop1_candidate(const void *arena, uint64_t arena_records, const uint32_t *off, const uint32_t *mask, const uint32_t *h,
                                            const uint32_t *tail, const uint32_t *c, const double *end, int64_t n_cases, int lanes, double *out_t,
                                            double *out_lat, void *stream) {
    if (!off || !mask || !h || !tail || !c || !end || !out_t || !out_lat) return (int)hipErrorInvalidValue;
    if (arena && arena_records && arena_records <= (1ull << 28) && (lanes == 8 || lanes == 16) && n_cases == 0) return (int)hipSuccess;
    const unsigned blocks = blocks_for(arena, arena_records, n_cases, lanes);
    if (!blocks) return (int)hipErrorInvalidValue;
    const double2 *a = (const double2 *)arena;
    if (lanes == 8)
        hipLaunchKernelGGL((drop_hop1_harness_kernel<8>), dim3(blocks), dim3(kWalkMaxBlock), 0, (hipStream_t)stream, a, arena_records, off, mask, h,
                           tail, c, end, n_cases, out_t, out_lat);
    else
        hipLaunchKernelGGL((drop_hop1_harness_kernel<16>), dim3(blocks), dim3(kWalkMaxBlock), 0, (hipStream_t)stream, a, arena_records, off, mask, h,
                           tail, c, end, n_cases, out_t, out_lat);
    return (int)hipGetLastError();
}
