// pcc_episodes.hip -- the episode ledger: per-env running episode totals over the [T][n_envs] rows of a rollout, every env's last
// finished episode, and per-member totals of the finished episodes (include/pcc_policy.h: pcc_episode_update_pop and its
// stand-alone form).
//
//   episode_walk_kernel   grid (G, n_members), 256 threads, G = ceil(n_m / 256): lane = env, member-local index blockIdx.x * 256 +
//                         tid (a member is cut into workgroups exactly as a launch over the member alone).  The lane walks its T
//                         steps in order: the reward and done loads are coalesced across the lanes, the step-record loads are one
//                         152-byte row per lane and step; four steps' loads are issued before the dependent additions (the loads
//                         are independent, only the accumulators are a chain).  carry / last are written by the lane that owns the
//                         env; the lane's partial {episodes, steps, per channel sum, sumsq, min, max} of the episodes it finished
//                         stays in registers, is summed over the wavefront by xor-shuffles in a fixed order, over the 4 wavefronts
//                         through LDS in index order, and goes to scratch[member][workgroup][2 + 4 C].
//   episode_merge_kernel  grid (n_members), 1024 threads: quantity q = tid % 64 of the 2 + 4 C, sub-lane tid / 64 combines a
//                         contiguous range of the member's partials in index order, a fixed tree in LDS combines the 16 sub-lanes,
//                         and the quantity's thread merges the batch into the member's row of totals -- nothing is written when
//                         the batch has no finished episode.
//
// An empty partial is {0, 0, per channel 0, 0, +inf, -inf}: neutral under +, fmin and fmax, so empty lanes, workgroups and
// sub-lanes need no special case.  No atomics, no hand-off between workgroups: the same inputs give the same bits.  A unit of its
// own (see pcc_obsnorm.hip: adding kernels to an existing unit moves the old kernels' schedules).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pcc_policy.h"
#include "pcc_sim.h"

namespace {

constexpr int kEpThreads = 256;
constexpr int kEpMaxChannels = 8;
constexpr int kEpMaxMembers = 1024;
constexpr int kEpQuantities = 2 + 4 * kEpMaxChannels;   // a partial of 8 channels
constexpr int kEpUnroll = 4;                            // steps whose loads are in flight together
constexpr int kEpMergeThreads = 1024;
constexpr int kEpMergeP = 64;                           // quantity lanes of the merge (>= kEpQuantities)
constexpr int kEpMergeSubs = kEpMergeThreads / kEpMergeP;

struct EpCols {
    int c[kEpMaxChannels - 1];   // the step-record column of channel 1 + k
};

// the kind of quantity q of a partial: 0 a sum (episodes, steps, sum, sumsq), 1 a minimum, 2 a maximum
__device__ __forceinline__ int ep_kind(int q) {
    const int k = (q - 2) & 3;
    return q < 2 || k < 2 ? 0 : k - 1;
}

__device__ __forceinline__ double ep_neutral(int kind) {
    return kind == 0 ? 0.0 : kind == 1 ? (double)INFINITY : -(double)INFINITY;
}

__device__ __forceinline__ double ep_combine(int kind, double a, double b) {
    return kind == 0 ? a + b : kind == 1 ? fmin(a, b) : fmax(a, b);
}

__global__ __launch_bounds__(kEpThreads) void episode_walk_kernel(const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                                                  const double *__restrict__ steps, EpCols cols, int C, int T,
                                                                  int64_t n_envs, int64_t n_m, double *__restrict__ carry,
                                                                  int32_t *__restrict__ carry_len, double *__restrict__ last,
                                                                  int32_t *__restrict__ last_len, double *__restrict__ scratch) {
    __shared__ double s_part[kEpThreads / 64][kEpQuantities];
    const int tid = threadIdx.x;
    const int64_t local = (int64_t)blockIdx.x * kEpThreads + tid;
    const bool live = local < n_m;
    const int64_t i = (int64_t)blockIdx.y * n_m + local;   // the env

    double run[kEpMaxChannels], p_sum[kEpMaxChannels], p_sq[kEpMaxChannels], p_min[kEpMaxChannels], p_max[kEpMaxChannels];
    double p_eps = 0.0, p_steps = 0.0;
    int32_t len = 0;
#pragma unroll
    for (int c = 0; c < kEpMaxChannels; c++) {
        run[c] = 0.0; p_sum[c] = 0.0; p_sq[c] = 0.0;
        p_min[c] = (double)INFINITY; p_max[c] = -(double)INFINITY;
    }
    if (live) {
        len = carry_len[i];
#pragma unroll
        for (int c = 0; c < kEpMaxChannels; c++)
            if (c < C) run[c] = carry[i * C + c];

        // one step: the additions, and the episode's end
        auto step = [&](const double (&x)[kEpMaxChannels], uint8_t d) {
#pragma unroll
            for (int c = 0; c < kEpMaxChannels; c++)
                if (c < C) run[c] += x[c];
            len += 1;
            if (d) {
                if (last_len) last_len[i] = len;
                p_eps += 1.0;
                p_steps += (double)len;
#pragma unroll
                for (int c = 0; c < kEpMaxChannels; c++) {
                    if (c < C) {
                        const double v = run[c];
                        if (last) last[i * C + c] = v;
                        p_sum[c] += v;
                        p_sq[c] += v * v;
                        p_min[c] = fmin(p_min[c], v);
                        p_max[c] = fmax(p_max[c], v);
                        run[c] = 0.0;
                    }
                }
                len = 0;
            }
        };
        auto load = [&](int t, double (&x)[kEpMaxChannels], uint8_t &d) {
            const int64_t at = (int64_t)t * n_envs + i;
            x[0] = (double)reward[at];
            d = done[at];
#pragma unroll
            for (int c = 1; c < kEpMaxChannels; c++)
                if (c < C) x[c] = steps[at * PCC_STEP_COLS + cols.c[c - 1]];
        };

        int t = 0;
        for (; t + kEpUnroll <= T; t += kEpUnroll) {
            double x[kEpUnroll][kEpMaxChannels];
            uint8_t d[kEpUnroll];
#pragma unroll
            for (int u = 0; u < kEpUnroll; u++) load(t + u, x[u], d[u]);
#pragma unroll
            for (int u = 0; u < kEpUnroll; u++) step(x[u], d[u]);
        }
        for (; t < T; t++) {
            double x[kEpMaxChannels];
            uint8_t d;
            load(t, x, d);
            step(x, d);
        }
        carry_len[i] = len;
#pragma unroll
        for (int c = 0; c < kEpMaxChannels; c++)
            if (c < C) carry[i * C + c] = run[c];
    }

    // the wavefront's lanes by xor-shuffles (every lane ends with the same value), then the 4 wavefronts in index order
    auto wave = [&](double v, int kind) {
        for (int d = 32; d >= 1; d >>= 1) v = ep_combine(kind, v, __shfl_xor(v, d));
        return v;
    };
    p_eps = wave(p_eps, 0);
    p_steps = wave(p_steps, 0);
#pragma unroll
    for (int c = 0; c < kEpMaxChannels; c++) {
        if (c < C) {
            p_sum[c] = wave(p_sum[c], 0);
            p_sq[c] = wave(p_sq[c], 0);
            p_min[c] = wave(p_min[c], 1);
            p_max[c] = wave(p_max[c], 2);
        }
    }
    if ((tid & 63) == 0) {
        double *w = s_part[tid >> 6];
        w[0] = p_eps;
        w[1] = p_steps;
#pragma unroll
        for (int c = 0; c < kEpMaxChannels; c++) {
            if (c < C) {
                w[2 + 4 * c] = p_sum[c];
                w[3 + 4 * c] = p_sq[c];
                w[4 + 4 * c] = p_min[c];
                w[5 + 4 * c] = p_max[c];
            }
        }
    }
    __syncthreads();
    const int Q = 2 + 4 * C;
    if (tid < Q) {
        const int kind = ep_kind(tid);
        double v = s_part[0][tid];
        for (int w = 1; w < kEpThreads / 64; w++) v = ep_combine(kind, v, s_part[w][tid]);
        scratch[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * Q + tid] = v;
    }
}

__global__ __launch_bounds__(kEpMergeThreads) void episode_merge_kernel(const double *__restrict__ scratch, int groups, int C,
                                                                        double *__restrict__ totals, int64_t totals_stride) {
    __shared__ double s_red[kEpMergeThreads];
    const int tid = threadIdx.x, q = tid & (kEpMergeP - 1), sub = tid / kEpMergeP;
    const int Q = 2 + 4 * C;
    const int kind = ep_kind(q);
    const double *part = scratch + (int64_t)blockIdx.x * groups * Q;
    const int per = (groups + kEpMergeSubs - 1) / kEpMergeSubs;
    const int g0 = sub * per, g1 = q < Q ? ((sub + 1) * per < groups ? (sub + 1) * per : groups) : 0;   // (an idle lane: no partial)
    double v = ep_neutral(kind);
    int g = g0;
    for (; g + 3 < g1; g += 4) {   // four partials' loads in flight, combined in index order
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = part[(int64_t)(g + u) * Q + q];
#pragma unroll
        for (int u = 0; u < 4; u++) v = ep_combine(kind, v, x[u]);
    }
    for (; g < g1; g++) v = ep_combine(kind, v, part[(int64_t)g * Q + q]);
    s_red[tid] = v;
    __syncthreads();
    for (int half = kEpMergeSubs >> 1; half >= 1; half >>= 1) {
        if (sub < half) s_red[tid] = ep_combine(kind, s_red[tid], s_red[tid + half * kEpMergeP]);
        __syncthreads();
    }
    // the batch into the member's row: nothing is written without a finished episode; the row's min / max are read only
    // when the row holds episodes
    const double batch_eps = s_red[0];
    double *row = totals + (int64_t)blockIdx.x * totals_stride;
    const bool writer = tid < Q && batch_eps > 0.0;
    const double row_eps = writer ? row[0] : 0.0;
    __syncthreads();   // (every writer has read the row's episodes before thread 0 writes them)
    if (writer) {
        const double b = s_red[tid];
        row[tid] = kind == 0 ? row[tid] + b : row_eps > 0.0 ? ep_combine(kind, row[tid], b) : b;
    }
}

}  // namespace

extern "C" int pcc_episode_scratch_doubles(int64_t n_envs, int n_members, int n_channels) {
    if (n_channels < 1 || n_channels > kEpMaxChannels || n_members < 1 || n_members > kEpMaxMembers || n_envs < 1 ||
        n_envs % n_members != 0)
        return -1;
    const int64_t groups = (n_envs / n_members + kEpThreads - 1) / kEpThreads;
    if (groups > 0x7fffffff / ((int64_t)n_members * (2 + 4 * n_channels))) return -1;
    return (int)(groups * n_members * (2 + 4 * n_channels));
}

extern "C" int pcc_episode_update_pop(const float *reward, const uint8_t *done, const double *steps, const int32_t *cols,
                                      int n_channels, int T, int64_t n_envs, int n_members, double *carry, int32_t *carry_len,
                                      double *last, int32_t *last_len, double *totals, int64_t totals_stride, double *scratch,
                                      void *stream) {
    // (every refusal comes before any HIP call: a host without a device gives the same answers)
    if (!reward || !done || !carry || !carry_len || !totals || !scratch) return -1;
    if (T < 1 || pcc_episode_scratch_doubles(n_envs, n_members, n_channels) < 0) return -1;
    if (totals_stride < 2 + 4 * (int64_t)n_channels) return -1;
    if (n_channels > 1 && (!steps || !cols)) return -1;
    if (n_envs > INT64_MAX / (PCC_STEP_COLS * (int64_t)sizeof(double)) / T) return -1;   // (no index below overflows)
    EpCols ec;
    for (int k = 0; k < kEpMaxChannels - 1; k++) {
        ec.c[k] = 0;
        if (k < n_channels - 1) {
            if (cols[k] < 0 || cols[k] >= PCC_STEP_COLS) return -1;
            ec.c[k] = cols[k];
        }
    }
    const int64_t n_m = n_envs / n_members;
    const int groups = (int)((n_m + kEpThreads - 1) / kEpThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(episode_walk_kernel, dim3((unsigned)groups, (unsigned)n_members), dim3(kEpThreads), 0, st, reward, done, steps,
                       ec, n_channels, T, n_envs, n_m, carry, carry_len, last, last_len, scratch);
    if (hipGetLastError() != hipSuccess) return -3;
    hipLaunchKernelGGL(episode_merge_kernel, dim3((unsigned)n_members), dim3(kEpMergeThreads), 0, st, scratch, groups, n_channels,
                       totals, totals_stride);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// The stand-alone form: a population of one (no twin kernels).
extern "C" int pcc_episode_update(const float *reward, const uint8_t *done, const double *steps, const int32_t *cols, int n_channels,
                                  int T, int64_t n_envs, double *carry, int32_t *carry_len, double *last, int32_t *last_len,
                                  double *totals, int64_t totals_stride, double *scratch, void *stream) {
    return pcc_episode_update_pop(reward, done, steps, cols, n_channels, T, n_envs, 1, carry, carry_len, last, last_len, totals,
                                  totals_stride, scratch, stream);
}
