// rtt_means_harness.hip -- TEST ONLY (tests/test_rtt_means.py), never part of libpcc_sim.so: rtt_means<8> and rtt_means<16> of
// pcc_retire_env.h, unchanged, on inputs the test chooses -- one group of G lanes per case, the group formed as retire_kernel
// forms it, the call under the divergence the product calls it under (a group without samples skips it while its neighbours in
// the wavefront make it).  A separate compilation of the same source: it holds the algorithm to numpy, not the product's
// machine code (tests/test_rtt_lengths.py holds that to the oracle at the same lengths).
#include <hip/hip_runtime.h>

#include "pcc_retire_env.h"

namespace {

template <int G>
__global__ __launch_bounds__(kWalkMaxBlock) void rtt_means_harness_kernel(const double2 *ring, uint32_t mask, const uint32_t *from,
                                                                          const uint32_t *n, const uint8_t *need_halves, const double *dl,
                                                                          int64_t n_cases, double *mean_all, double *lat_inc) {
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    Group g;
    g.lane = tid & (uint32_t)(G - 1);
    g.shift = lane & ~(uint32_t)(G - 1);
    const int64_t c = (int64_t)blockIdx.x * (kWalkMaxBlock / G) + tid / (uint32_t)G;
    uint32_t acked = 0;
    if (c < n_cases) acked = n[c];
    if (acked > 0) {   // (group-uniform; wavefront-divergent)
        double lat, inc;
        rtt_means<G>(g, ring, mask, from[c], acked, dl[c], need_halves[c] != 0, lat, inc);
        if (g.lane == 0) {
            mean_all[c] = lat;
            lat_inc[c] = inc;
        }
    }
}

}  // namespace

// ring: `ring_records` double2 records (a power of two; only .y is read); the four case arrays and the two outputs have n_cases
// entries (device memory); lanes: 8 or 16 per case.  Returns the HIP error code (hipErrorInvalidValue for arguments it refuses).
extern "C" int pcc_test_rtt_means(const void *ring, uint32_t ring_records, const uint32_t *from, const uint32_t *n, const uint8_t *need_halves,
                                  const double *dl, int64_t n_cases, int lanes, double *mean_all, double *lat_inc, void *stream) {
    if (!ring || ring_records == 0 || (ring_records & (ring_records - 1)) != 0 || ring_records > (1u << 28)) return (int)hipErrorInvalidValue;
    if ((lanes != 8 && lanes != 16) || n_cases < 0 || !from || !n || !need_halves || !dl || !mean_all || !lat_inc) return (int)hipErrorInvalidValue;
    if (n_cases == 0) return (int)hipSuccess;
    const int64_t per_block = kWalkMaxBlock / lanes;
    const int64_t blocks = (n_cases + per_block - 1) / per_block;
    if (blocks > 0x7FFFFFFF) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const double2 *r = (const double2 *)ring;
    if (lanes == 8)
        hipLaunchKernelGGL((rtt_means_harness_kernel<8>), dim3((unsigned)blocks), dim3(kWalkMaxBlock), 0, st, r, ring_records - 1u, from, n,
                           need_halves, dl, n_cases, mean_all, lat_inc);
    else
        hipLaunchKernelGGL((rtt_means_harness_kernel<16>), dim3((unsigned)blocks), dim3(kWalkMaxBlock), 0, st, r, ring_records - 1u, from, n,
                           need_halves, dl, n_cases, mean_all, lat_inc);
    return (int)hipGetLastError();
}
