// pcc_rewnorm.hip -- reward normalisation: the running per-member variance of the discounted return of every env over the
// [T][n_envs] reward and done rows of a rollout, and the scaled, clipped reward rows the advantage estimation reads
// (include/pcc_policy.h: pcc_return_stats_update_pop, pcc_reward_normalise_pop and their stand-alone forms).
//
//   return_walk_kernel       grid (G, n_members), 256 threads, G = ceil(n_m / 256): lane = env, member-local index blockIdx.x * 256
//                            + tid (a member is cut into workgroups exactly as a launch over the member alone).  The lane walks its
//                            T steps in order, R = R * gamma + r, sample, R = 0 after a done: the reward and done loads are coalesced
//                            across the lanes, eight steps' loads are issued before the dependent chain.  A lane carries ONE float64
//                            pair {sum, sum of squares} of R - k, k = the lane's first sample (no cancellation against a large mean,
//                            no division per sample), which gives the lane's {n = T, mean, m2}.  The lanes of a wavefront are merged
//                            by Chan's formula in a down-shuffle tree (lane 0 holds the result), the 4 wavefronts through LDS in
//                            index order, and the workgroup's {n, mean, m2} go to scratch[member][workgroup][3].
//   return_merge_kernel      grid (n_members), 256 threads: sub-lane tid sums a contiguous range of the member's partials in index
//                            order -- count-weighted sums of the partial means' distances from partial 0's and of their squares, no
//                            division per partial -- a fixed tree in LDS combines the sub-lanes, and thread 0 merges the batch into
//                            the member's row of stats by Chan's formula and writes scale.
//   reward_normalise_kernel  grid (ceil(n_m / 1024), n_members, min(T, 65535)), 256 threads: four consecutive envs per thread (one
//                            float4 when every member's run of every row is 16-byte aligned), rows blockIdx.z, + gridDim.z, ...
//
// An empty partial is {0, 0, 0}: chan_merge leaves the other side as it is, so the idle lanes of a member's last workgroup need no
// special case.  No atomics, no hand-off between workgroups: the same inputs give the same bits.  A unit of its own (see
// pcc_obsnorm.hip: adding kernels to an existing unit moves the old kernels' schedules).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcc_policy.h"

namespace {

constexpr int kRetThreads = 256;
constexpr int kRetMaxMembers = 1024;
constexpr int kRetUnroll = 8;        // steps whose loads are in flight together
constexpr int kRetHyperCols = 8;     // a row of `hyper`
constexpr int kRetHyperGamma = 3;    // ... and the column pcc_gae_pop reads gamma from

// Chan et al.'s pairwise update: (na, ma, qa) takes (nb, mb, qb) in; an empty side leaves the other as it is
__device__ __forceinline__ void chan_merge(double &na, double &ma, double &qa, double nb, double mb, double qb) {
    if (nb == 0.0) return;
    if (na == 0.0) {
        na = nb; ma = mb; qa = qb;
        return;
    }
    const double n = na + nb, d = mb - ma;
    ma = ma + d * nb / n;
    qa = qa + qb + d * d * na * nb / n;
    na = n;
}

__global__ __launch_bounds__(kRetThreads) void return_walk_kernel(const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                                                  int T, int64_t n_envs, int64_t n_m, const float *__restrict__ hyper,
                                                                  float gamma, double *__restrict__ ret_carry,
                                                                  double *__restrict__ scratch) {
    __shared__ double s_part[kRetThreads / 64][3];
    const int tid = threadIdx.x;
    const int64_t local = (int64_t)blockIdx.x * kRetThreads + tid;
    const bool live = local < n_m;
    const int64_t i = (int64_t)blockIdx.y * n_m + local;   // the env
    const double g = (double)(hyper ? hyper[(int64_t)blockIdx.y * kRetHyperCols + kRetHyperGamma] : gamma);

    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    if (live) {
        double R = ret_carry[i], k = 0.0, s = 0.0, q = 0.0;
        // one step: the recurrence, the sample, the episode's end
        auto step = [&](float r, uint8_t d, bool first) {
            R = R * g + (double)r;
            if (first) k = R;
            const double x = R - k;
            s += x; q += x * x;
            if (d) R = 0.0;
        };
        const float *rp = reward + i;
        const uint8_t *dp = done + i;
        {   // step 0 sets k
            step(rp[0], dp[0], true);
        }
        int t = 1;
        for (; t + kRetUnroll <= T; t += kRetUnroll) {
            float r[kRetUnroll];
            uint8_t d[kRetUnroll];
#pragma unroll
            for (int u = 0; u < kRetUnroll; u++) {
                r[u] = rp[(int64_t)(t + u) * n_envs];
                d[u] = dp[(int64_t)(t + u) * n_envs];
            }
#pragma unroll
            for (int u = 0; u < kRetUnroll; u++) step(r[u], d[u], false);
        }
        for (; t < T; t++) step(rp[(int64_t)t * n_envs], dp[(int64_t)t * n_envs], false);
        ret_carry[i] = R;
        cnt = (double)T;
        mean = k + s / cnt;
        const double dev = q - s * s / cnt;
        m2 = dev > 0.0 ? dev : 0.0;   // (a sum of squared deviations: rounding must not make it negative)
    }

    // the wavefront's lanes in a down-shuffle tree: lane 0 ends with the wavefront's moments (what the other lanes hold is not used)
    for (int d = 32; d >= 1; d >>= 1) {
        const double nb = __shfl_down(cnt, d), mb = __shfl_down(mean, d), qb = __shfl_down(m2, d);
        chan_merge(cnt, mean, m2, nb, mb, qb);
    }
    if ((tid & 63) == 0) {
        double *w = s_part[tid >> 6];
        w[0] = cnt; w[1] = mean; w[2] = m2;
    }
    __syncthreads();
    if (tid == 0) {   // ... then the 4 wavefronts in index order
        for (int w = 1; w < kRetThreads / 64; w++) chan_merge(cnt, mean, m2, s_part[w][0], s_part[w][1], s_part[w][2]);
        double *out = scratch + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        out[0] = cnt; out[1] = mean; out[2] = m2;
    }
}

__global__ __launch_bounds__(kRetThreads) void return_merge_kernel(const double *__restrict__ scratch, int groups,
                                                                   double *__restrict__ stats, int64_t stat_stride,
                                                                   float *__restrict__ scale, double eps) {
    __shared__ double s_red[4][kRetThreads];
    const int tid = threadIdx.x;
    const double *part = scratch + (int64_t)blockIdx.x * groups * 3;
    const int per = (groups + kRetThreads - 1) / kRetThreads;
    const int g0 = tid * per < groups ? tid * per : groups, g1 = g0 + per < groups ? g0 + per : groups;
    // The batch's moments from the partials' {count, mean, m2} in one pass in index order, no division per partial: with d_g the
    // distance of partial g's mean from partial 0's, mean = k + sum(count_g d_g) / n and m2 = sum(m2_g) + sum(count_g d_g^2) -
    // sum(count_g d_g)^2 / n.  (Every partial of a member holds at least one env: no count is 0.)
    const double k = part[1];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int g = g0; g < g1; g++) {
        const double c = part[(int64_t)g * 3], d = part[(int64_t)g * 3 + 1] - k;
        a0 += c; a1 += c * d; a2 += c * (d * d); a3 += part[(int64_t)g * 3 + 2];
    }
    s_red[0][tid] = a0; s_red[1][tid] = a1; s_red[2][tid] = a2; s_red[3][tid] = a3;
    __syncthreads();
    for (int half = kRetThreads >> 1; half >= 1; half >>= 1) {   // a fixed tree over the sub-lanes
        if (tid < half) {
#pragma unroll
            for (int j = 0; j < 4; j++) s_red[j][tid] += s_red[j][tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) {   // the batch into the member's running row
        const double nb = s_red[0][0], s1 = s_red[1][0], s2 = s_red[2][0], s3 = s_red[3][0];
        const double between = s2 - s1 * s1 / nb;
        const double mb = k + s1 / nb, qb = s3 + (between > 0.0 ? between : 0.0);
        double *row = stats + (int64_t)blockIdx.x * stat_stride;
        double cnt = row[0], mean = row[1], m2 = row[2];
        chan_merge(cnt, mean, m2, nb, mb, qb);
        row[0] = cnt; row[1] = mean; row[2] = m2;
        if (scale) scale[blockIdx.x] = (float)(1.0 / sqrt(m2 / cnt + eps));
    }
}

__global__ __launch_bounds__(kRetThreads) void reward_normalise_kernel(const float *reward, int T, int64_t n_envs, int64_t n_m,
                                                                       const float *__restrict__ scale, float clip, float *out,
                                                                       int vec_ok) {
    const int64_t e = ((int64_t)blockIdx.x * kRetThreads + threadIdx.x) * 4;   // the first of this thread's envs of the member
    if (e >= n_m) return;
    const float s = scale[blockIdx.y];
    const int cnt = n_m - e < 4 ? (int)(n_m - e) : 4;
    const bool vec = vec_ok && cnt == 4;
    const int64_t col = (int64_t)blockIdx.y * n_m + e;
    for (int t = blockIdx.z; t < T; t += gridDim.z) {
        const int64_t at = (int64_t)t * n_envs + col;
        if (vec) {
            float4 v = *reinterpret_cast<const float4 *>(reward + at);
            v.x = fminf(fmaxf(v.x * s, -clip), clip);
            v.y = fminf(fmaxf(v.y * s, -clip), clip);
            v.z = fminf(fmaxf(v.z * s, -clip), clip);
            v.w = fminf(fmaxf(v.w * s, -clip), clip);
            *reinterpret_cast<float4 *>(out + at) = v;
        } else {
            for (int j = 0; j < cnt; j++) out[at + j] = fminf(fmaxf(reward[at + j] * s, -clip), clip);
        }
    }
}

// the member's workgroups of the walk; -1 outside the domain (no index of the kernels overflows inside it)
int64_t ret_groups(int T, int64_t n_envs, int n_members) {
    if (T < 1 || n_envs < 1 || n_members < 1 || n_members > kRetMaxMembers || n_envs % n_members != 0) return -1;
    if (n_envs > INT64_MAX / (int64_t)sizeof(double) / T) return -1;
    const int64_t groups = (n_envs / n_members + kRetThreads - 1) / kRetThreads;
    if (groups > 0x7fffffff / (3 * (int64_t)n_members)) return -1;
    return groups;
}

int return_update(const float *reward, const uint8_t *done, int T, int64_t n_envs, int n_members, const float *hyper, float gamma,
                  double *ret_carry, double *stats, int64_t stat_stride, float *scale, double eps, double *scratch, void *stream) {
    // (every refusal comes before any HIP call: a host without a device gives the same answers)
    if (!reward || !done || !ret_carry || !stats || !scratch) return -1;
    const int64_t groups = ret_groups(T, n_envs, n_members);
    if (groups < 0 || stat_stride < 3 || !(eps >= 0.0)) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(return_walk_kernel, dim3((unsigned)groups, (unsigned)n_members), dim3(kRetThreads), 0, st, reward, done, T,
                       n_envs, n_envs / n_members, hyper, gamma, ret_carry, scratch);
    if (hipGetLastError() != hipSuccess) return -3;
    hipLaunchKernelGGL(return_merge_kernel, dim3((unsigned)n_members), dim3(kRetThreads), 0, st, scratch, (int)groups, stats,
                       stat_stride, scale, eps);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

extern "C" int pcc_return_scratch_doubles(int T, int64_t n_envs, int n_members) {
    const int64_t groups = ret_groups(T, n_envs, n_members);
    return groups < 0 ? -1 : (int)(groups * n_members * 3);
}

extern "C" int pcc_return_stats_update_pop(const float *reward, const uint8_t *done, int T, int64_t n_envs, int n_members,
                                           const float *hyper, double *ret_carry, double *stats, int64_t stat_stride, float *scale,
                                           double eps, double *scratch, void *stream) {
    if (!hyper) return -1;
    return return_update(reward, done, T, n_envs, n_members, hyper, 0.0f, ret_carry, stats, stat_stride, scale, eps, scratch, stream);
}

extern "C" int pcc_reward_normalise_pop(const float *reward, int T, int64_t n_envs, int n_members, const float *scale, float clip,
                                        float *out, void *stream) {
    if (!reward || !scale || !out) return -1;
    if (ret_groups(T, n_envs, n_members) < 0 || !(clip > 0.0f)) return -1;
    const int64_t n_m = n_envs / n_members, blocks = (n_m + 4 * kRetThreads - 1) / (4 * kRetThreads);
    // float4 when every member's run of every row starts on 16 bytes; else float by float
    const int vec_ok = n_m % 4 == 0 && ((reinterpret_cast<uintptr_t>(reward) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
    hipLaunchKernelGGL(reward_normalise_kernel, dim3((unsigned)blocks, (unsigned)n_members, (unsigned)(T < 65535 ? T : 65535)),
                       dim3(kRetThreads), 0, static_cast<hipStream_t>(stream), reward, T, n_envs, n_m, scale, clip, out, vec_ok);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// The stand-alone forms: a population of one (no twin kernels); gamma comes as an argument, not from hyper.
extern "C" int pcc_return_stats_update(const float *reward, const uint8_t *done, int T, int64_t n_envs, float gamma, double *ret_carry,
                                       double *stats, float *scale, double eps, double *scratch, void *stream) {
    return return_update(reward, done, T, n_envs, 1, nullptr, gamma, ret_carry, stats, 3, scale, eps, scratch, stream);
}

extern "C" int pcc_reward_normalise(const float *reward, int T, int64_t n_envs, const float *scale, float clip, float *out,
                                    void *stream) {
    return pcc_reward_normalise_pop(reward, T, n_envs, 1, scale, clip, out, stream);
}
