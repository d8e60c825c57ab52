// pcc_objective.hip -- reward objectives: the [T][n_envs] reward rows of a rollout recomputed from its float64 step records under
// per-member weights over six of their metrics, and the per-member sums of the weighted terms (include/pcc_policy.h:
// pcc_reward_objective_pop and its stand-alone form).
//
//   objective_walk_kernel   grid (G, n_members), 256 threads, G = ceil(n_m / 256): lane = env, member-local index blockIdx.x * 256 +
//                           tid (a member is cut into workgroups exactly as a launch over the member alone).  The member's six
//                           weights are read once and are the same in every lane of the workgroup: a term whose weight is 0 is
//                           skipped by a uniform branch, its column is never loaded.  The lane walks its T steps in order: the record
//                           loads are one 152-byte row per lane and step (as episode_walk_kernel's), four steps' loads are issued
//                           before the arithmetic, the reward store is coalesced across the lanes.  The lane's partial {six term
//                           sums, the sum of the float32 rewards} stays in registers, is summed over the wavefront in a
//                           down-shuffle tree (lane 0 holds the result), over the 4 wavefronts through LDS in index order, and goes
//                           to scratch[member][workgroup][7].
//   objective_merge_kernel  grid (n_members), 256 threads: sub-lane tid sums a contiguous range of the member's partials in index
//                           order from 0.0, a fixed halving tree in LDS combines the sub-lanes, and the threads 0 .. 6 write the
//                           member's row of sums.
//
// An idle lane's partial is seven zeros.  No atomics, no hand-off between workgroups: the same inputs give the same bits.  A unit of
// its own (see pcc_obsnorm.hip: adding kernels to an existing unit moves the old kernels' schedules).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcc_policy.h"
#include "pcc_sim.h"

namespace {

constexpr int kObjThreads = 256;
constexpr int kObjMaxMembers = 1024;
constexpr int kObjUnroll = 4;                   // steps whose loads are in flight together
constexpr int kObjQuantities = PCC_OBJ_TERMS + 1;   // a partial: the term sums, then the reward sum
constexpr double kObjRewardScale = 0.001;       // the env's kRewardScale (csrc/pcc_dev.h)
constexpr double kObjPacketBits = 12000.0;      // 8 * 1500: the env divides a rate by the bits of a packet

// the metric of term k, as a step-record column
__device__ __forceinline__ constexpr int obj_column(int k) {
    return PCC_COL_METRIC0 + (k == PCC_OBJ_THROUGHPUT          ? PCC_M_RECV_RATE
                              : k == PCC_OBJ_LATENCY           ? PCC_M_AVG_LATENCY
                              : k == PCC_OBJ_LOSS              ? PCC_M_LOSS_RATIO
                              : k == PCC_OBJ_LATENCY_INFLATION ? PCC_M_SENT_LATENCY_INFLATION
                              : k == PCC_OBJ_LATENCY_RATIO     ? PCC_M_LATENCY_RATIO
                                                               : PCC_M_SEND_RATE);
}

// weighted term k of a sample: the env's own operations in its order (a rate: the product, then the division)
__device__ __forceinline__ double obj_term(int k, double w, double m) {
    return (k == PCC_OBJ_THROUGHPUT || k == PCC_OBJ_SEND_RATE) ? (w * m) / kObjPacketBits : w * m;
}

__global__ __launch_bounds__(kObjThreads) void objective_walk_kernel(const double *__restrict__ steps, int T, int64_t n_envs,
                                                                     int64_t n_m, const double *__restrict__ weights,
                                                                     float *__restrict__ reward_out, double *__restrict__ scratch) {
    __shared__ double s_part[kObjThreads / 64][kObjQuantities];
    const int tid = threadIdx.x;
    const int64_t local = (int64_t)blockIdx.x * kObjThreads + tid;
    const bool live = local < n_m;
    const int64_t i = (int64_t)blockIdx.y * n_m + local;   // the env

    double w[PCC_OBJ_TERMS];
    bool on[PCC_OBJ_TERMS];
#pragma unroll
    for (int k = 0; k < PCC_OBJ_TERMS; k++) {
        w[k] = weights[(int64_t)blockIdx.y * PCC_OBJ_TERMS + k];
        on[k] = w[k] != 0.0;   // (the same in every lane; a NaN weight is refused by the caller, it would count as on)
    }

    double p[kObjQuantities];
#pragma unroll
    for (int q = 0; q < kObjQuantities; q++) p[q] = 0.0;

    if (live) {
        const double *row0 = steps + i * PCC_STEP_COLS;
        const int64_t row_stride = n_envs * PCC_STEP_COLS;
        float *out = reward_out + i;

        auto load = [&](int t, double (&x)[PCC_OBJ_TERMS]) {
            const double *row = row0 + (int64_t)t * row_stride;
#pragma unroll
            for (int k = 0; k < PCC_OBJ_TERMS; k++)
                if (on[k]) x[k] = row[obj_column(k)];
        };
        // one sample: the terms in index order, the first included one starts the sum, the scale, the cast
        auto sample = [&](int t, const double (&x)[PCC_OBJ_TERMS]) {
            double acc = 0.0;
            bool any = false;
#pragma unroll
            for (int k = 0; k < PCC_OBJ_TERMS; k++) {
                if (on[k]) {
                    const double term = obj_term(k, w[k], x[k]);
                    acc = any ? acc + term : term;
                    any = true;
                    p[k] += term;
                }
            }
            const float r = (float)(acc * kObjRewardScale);
            out[(int64_t)t * n_envs] = r;
            p[PCC_OBJ_TERMS] += (double)r;
        };

        int t = 0;
        for (; t + kObjUnroll <= T; t += kObjUnroll) {
            double x[kObjUnroll][PCC_OBJ_TERMS];
#pragma unroll
            for (int u = 0; u < kObjUnroll; u++) load(t + u, x[u]);
#pragma unroll
            for (int u = 0; u < kObjUnroll; u++) sample(t + u, x[u]);
        }
        for (; t < T; t++) {
            double x[PCC_OBJ_TERMS];
            load(t, x);
            sample(t, x);
        }
    }

    // the wavefront's lanes in a down-shuffle tree: lane 0 ends with the wavefront's sums (what the other lanes hold is not used)
#pragma unroll
    for (int q = 0; q < kObjQuantities; q++)
        for (int d = 32; d >= 1; d >>= 1) p[q] += __shfl_down(p[q], d);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < kObjQuantities; q++) s_part[tid >> 6][q] = p[q];
    }
    __syncthreads();
    if (tid == 0) {   // ... then the 4 wavefronts in index order
        double *dst = scratch + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kObjQuantities;
#pragma unroll
        for (int q = 0; q < kObjQuantities; q++) {
            double v = p[q];
            for (int wv = 1; wv < kObjThreads / 64; wv++) v += s_part[wv][q];
            dst[q] = v;
        }
    }
}

__global__ __launch_bounds__(kObjThreads) void objective_merge_kernel(const double *__restrict__ scratch, int groups,
                                                                      double *__restrict__ sums) {
    __shared__ double s_red[kObjQuantities][kObjThreads];
    const int tid = threadIdx.x;
    const double *part = scratch + (int64_t)blockIdx.x * groups * kObjQuantities;
    const int per = (groups + kObjThreads - 1) / kObjThreads;
    const int g0 = (int64_t)tid * per < groups ? tid * per : groups, g1 = g0 + per < groups ? g0 + per : groups;
    double a[kObjQuantities];
#pragma unroll
    for (int q = 0; q < kObjQuantities; q++) a[q] = 0.0;
    for (int g = g0; g < g1; g++) {
#pragma unroll
        for (int q = 0; q < kObjQuantities; q++) a[q] += part[(int64_t)g * kObjQuantities + q];
    }
#pragma unroll
    for (int q = 0; q < kObjQuantities; q++) s_red[q][tid] = a[q];
    __syncthreads();
    for (int half = kObjThreads >> 1; half >= 1; half >>= 1) {   // a fixed tree over the sub-lanes
        if (tid < half) {
#pragma unroll
            for (int q = 0; q < kObjQuantities; q++) s_red[q][tid] += s_red[q][tid + half];
        }
        __syncthreads();
    }
    if (tid < kObjQuantities) sums[(int64_t)blockIdx.x * kObjQuantities + tid] = s_red[tid][0];
}

// the member's workgroups of the walk; -1 outside the domain (no index of the kernels overflows inside it)
int64_t obj_groups(int T, int64_t n_envs, int n_members) {
    if (T < 1 || n_envs < 1 || n_members < 1 || n_members > kObjMaxMembers || n_envs % n_members != 0) return -1;
    if (n_envs > INT64_MAX / (PCC_STEP_COLS * (int64_t)sizeof(double)) / T) return -1;
    const int64_t groups = (n_envs / n_members + kObjThreads - 1) / kObjThreads;
    if (groups > 0x7fffffff / (kObjQuantities * (int64_t)n_members)) return -1;
    return groups;
}

}  // namespace

extern "C" int pcc_objective_scratch_doubles(int T, int64_t n_envs, int n_members) {
    const int64_t groups = obj_groups(T, n_envs, n_members);
    return groups < 0 ? -1 : (int)(groups * n_members * kObjQuantities);
}

extern "C" int pcc_reward_objective_pop(const double *steps, int T, int64_t n_envs, int n_members, const double *weights,
                                        float *reward_out, double *sums, double *scratch, void *stream) {
    // (every refusal comes before any HIP call: a host without a device gives the same answers)
    if (!steps || !weights || !reward_out || !scratch) return -1;
    const int64_t groups = obj_groups(T, n_envs, n_members);
    if (groups < 0) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(objective_walk_kernel, dim3((unsigned)groups, (unsigned)n_members), dim3(kObjThreads), 0, st, steps, T, n_envs,
                       n_envs / n_members, weights, reward_out, scratch);
    if (hipGetLastError() != hipSuccess) return -3;
    if (!sums) return 0;
    hipLaunchKernelGGL(objective_merge_kernel, dim3((unsigned)n_members), dim3(kObjThreads), 0, st, scratch, (int)groups, sums);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// The stand-alone form: a population of one (no twin kernels).
extern "C" int pcc_reward_objective(const double *steps, int T, int64_t n_envs, const double *weights, float *reward_out, double *sums,
                                    double *scratch, void *stream) {
    return pcc_reward_objective_pop(steps, T, n_envs, 1, weights, reward_out, sums, scratch, stream);
}
