// pcc_pbt.hip -- the step between two generations of a population (include/pcc_policy.h: pcc_pbt_evolve):
// truncation selection, copy and perturb of population-based training (Jaderberg et al. 2017) on the device-resident
// [members][param_stride] blocks of PopulationPPO, as ONE launch with no copy to the host and no synchronise.
//
//   pbt_evolve_kernel   grid (ceil(n_params / 1024), n_members), 256 threads: blockIdx.y = member m.  Every workgroup stages the
//                       scores in LDS (8 KB at the member limit) and counts the members better than m: its rank.  A survivor's
//                       x = 0 workgroup writes parent_out / rank_out and the whole workgroup leaves.  A replaced member draws
//                       its source's rank j from Philox (counter (m, generation, 0, 0)), finds the member of rank j -- thread t
//                       ranks the candidates t, t + 256, ...: K^2 / 256 compares per thread, 4 096 at K = 1024 -- and copies its
//                       1 024-float chunk of the three rows as float4 (rows are 256-byte aligned); a tail of n_params % 4 floats
//                       goes as scalars so that the padding is never touched.  The x = 0 workgroup writes the hyper row.
//
// Every workgroup of a member derives the same rank, source and draw from the same inputs: no workgroup waits for another, and
// nothing is communicated inside the launch.  A unit of its own: adding kernels to an existing unit moves the old kernels'
// schedules, and tests/test_ppo_shapes.py pins those.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcc_dev.h"   // philox4x32_10: the simulator's, not another copy
#include "pcc_policy.h"

namespace {

constexpr int kPbtThreads = 256;
constexpr int kPbtChunk = 4 * kPbtThreads;   // floats of a row per workgroup: one float4 per thread
constexpr int kPbtMaxMembers = 1024;
constexpr int kHyperCols = 8;

// the contract's ordering: a NaN score is worse than any number, equal scores (+0.0 and -0.0 too) go by index
__device__ __forceinline__ bool pbt_better(double sa, int a, double sb, int b) {
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return nb;
    if (!na && sa != sb) return sa > sb;
    return a < b;
}

// the sum of every thread's (a, b) over the workgroup, to every thread; red: 2 * 4 ints of LDS.  All 256 threads call it.
__device__ __forceinline__ void pbt_block_sum2(int &a, int &b, int *red) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_xor(a, d);
        b += __shfl_xor(b, d);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave] = a;
        red[4 + wave] = b;
    }
    __syncthreads();
    a = red[0] + red[1] + red[2] + red[3];
    b = red[4] + red[5] + red[6] + red[7];
}

__global__ __launch_bounds__(kPbtThreads) void pbt_evolve_kernel(const double *__restrict__ score, int n_members, int n_cut,
                                                                 float *params, float *adam_m, float *adam_v, int64_t param_stride,
                                                                 int64_t n_params, int vec_ok, float *hyper,
                                                                 const float *__restrict__ explore, uint32_t key0, uint32_t key1,
                                                                 uint32_t generation, int32_t *__restrict__ parent_out,
                                                                 int32_t *__restrict__ rank_out) {
    __shared__ double s_score[kPbtMaxMembers];
    __shared__ int s_red[8];
    __shared__ int s_src;
    const int tid = threadIdx.x, mb = blockIdx.y;
    for (int i = tid; i < n_members; i += kPbtThreads) s_score[i] = score[i];
    if (tid == 0) s_src = mb;   // (always a valid row; the search below overwrites it)
    __syncthreads();

    // rank[mb] = the number of members better than mb; n_valid = the number of scores that are numbers
    const double my = s_score[mb];
    int better = 0, valid = 0;
    for (int i = tid; i < n_members; i += kPbtThreads) {
        const double s = s_score[i];
        valid += s == s ? 1 : 0;
        better += i != mb && pbt_better(s, i, my, mb) ? 1 : 0;
    }
    pbt_block_sum2(better, valid, s_red);
    const int rank = better, n_src = n_cut < valid ? n_cut : valid;
    const bool lead = blockIdx.x == 0 && tid == 0;

    // Sources have rank < n_src <= n_cut <= n_members / 2 and replaced members rank >= n_members - n_cut >= n_members / 2 (2 n_cut
    // <= n_members is the host's check): the two sets are disjoint, so no row is both read and written in this launch, and
    // the order in which the workgroups run does not matter.
    if (n_src <= 0 || rank < n_members - n_cut) {   // a survivor: nothing of its rows is written (the whole workgroup leaves)
        if (lead) {
            if (parent_out) parent_out[mb] = mb;
            if (rank_out) rank_out[mb] = rank;
        }
        return;
    }

    uint32_t w[4];
    philox4x32_10((uint32_t)mb, generation, 0u, 0u, key0, key1, w);
    const int j = (int)(((uint64_t)w[0] * (uint64_t)(uint32_t)n_src) >> 32);   // uniform in [0, n_src)
    for (int c = tid; c < n_members; c += kPbtThreads) {   // the member of rank j: exactly one candidate has it (ranks are a permutation)
        const double sc = s_score[c];
        int r = 0;
        for (int i = 0; i < n_members; i++) r += i != c && pbt_better(s_score[i], i, sc, c) ? 1 : 0;
        if (r == j) s_src = c;
    }
    __syncthreads();
    const int p = s_src;

    // floats [0, n_params) of row p -> row mb, this workgroup's 1 024 of them
    const int64_t src = (int64_t)p * param_stride, dst = (int64_t)mb * param_stride;
    const int64_t e = (int64_t)blockIdx.x * kPbtChunk + 4 * tid;
    if (vec_ok && e + 4 <= n_params) {
        *reinterpret_cast<float4 *>(params + dst + e) = *reinterpret_cast<const float4 *>(params + src + e);
        *reinterpret_cast<float4 *>(adam_m + dst + e) = *reinterpret_cast<const float4 *>(adam_m + src + e);
        *reinterpret_cast<float4 *>(adam_v + dst + e) = *reinterpret_cast<const float4 *>(adam_v + src + e);
    } else {
        for (int64_t q = e; q < e + 4 && q < n_params; q++) {   // the tail of n_params % 4 floats (or blocks that are not 16-byte aligned)
            params[dst + q] = params[src + q];
            adam_m[dst + q] = adam_m[src + q];
            adam_v[dst + q] = adam_v[src + q];
        }
    }

    if (blockIdx.x == 0) {
        if (tid < kHyperCols) {   // the parent's value times one of two factors (bit tid of the second Philox word), clamped
            const float *ex = explore + 4 * tid;
            const float f = (w[1] >> tid) & 1u ? ex[1] : ex[0];
            const float x = hyper[(int64_t)p * kHyperCols + tid] * f;
            hyper[(int64_t)mb * kHyperCols + tid] = fminf(fmaxf(x, ex[2]), ex[3]);
        }
        if (tid == 0) {
            if (parent_out) parent_out[mb] = p;
            if (rank_out) rank_out[mb] = rank;
        }
    }
}

}  // namespace

extern "C" int pcc_pbt_evolve(const double *score, int n_members, int n_cut, float *params, float *adam_m, float *adam_v,
                              int64_t param_stride, int64_t n_params, float *hyper, const float *explore, uint64_t seed,
                              uint32_t generation, int32_t *parent_out, int32_t *rank_out, void *stream) {
    // (every refusal comes before any HIP call: a host without a device gives the same answers)
    if (!score || !params || !adam_m || !adam_v || !hyper || !explore) return -1;
    if (n_members < 1 || n_members > kPbtMaxMembers || n_cut < 0 || 2 * (int64_t)n_cut > n_members) return -1;
    if (param_stride % 64 != 0 || n_params < 1 || n_params > param_stride) return -1;
    const int64_t chunks = (n_params + kPbtChunk - 1) / kPbtChunk;
    if (chunks > 0x7fffffff) return -1;
    // rows are 256-byte aligned when the blocks are (any device allocation is); a block that is not goes float by float
    const int vec_ok = ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(adam_m) | reinterpret_cast<uintptr_t>(adam_v)) & 15u) == 0;
    hipLaunchKernelGGL(pbt_evolve_kernel, dim3((unsigned)chunks, (unsigned)n_members), dim3(kPbtThreads), 0,
                       static_cast<hipStream_t>(stream), score, n_members, n_cut, params, adam_m, adam_v, param_stride, n_params, vec_ok,
                       hyper, explore, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), generation, parent_out, rank_out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
