// pcc_obsnorm.hip -- running per-member, per-feature moments of the observation rows and the normalised rows the policy kernels
// read (include/pcc_policy.h: pcc_obs_stats_update_pop, pcc_obs_normalise_pop and their stand-alone forms).
//
//   obs_moments_kernel    grid (G, n_members), 256 threads.  A member's n = T * n_m rows are cut into G chunks of `chunk` rows
//                         (obs_cut: a function of T, n_m and obs_dim alone, so a member is cut exactly as a launch over the
//                         member alone).  P = the next power of two >= obs_dim; thread tid is feature tid % P of row lane
//                         tid / P: a lane always sees the same feature, the active lanes of a wavefront load one contiguous run,
//                         and a lane carries ONE float64 pair {sum, sum of squares} of x - k, k = the chunk's first value of its
//                         feature (the differences are exact in float64; no cancellation against a large mean).  The row lanes
//                         are summed by xor-shuffles in a fixed order, the wavefronts through 8 KB of LDS in index order, and
//                         the chunk's {mean, m2} go to scratch[member][chunk][2 * obs_dim].
//   obs_merge_kernel      grid (n_members), 256 threads: feature tid % P, sub-lane tid / P sums a contiguous range of the chunks
//                         in index order -- count-weighted sums of the chunk means' distances from chunk 0's and of their squares,
//                         no division per chunk -- a tree over the sub-lanes in LDS combines those, and the feature's thread
//                         merges the batch into the member's row of stats by Chan's formula and writes norm.
//   obs_normalise_kernel  grid (ceil(n_m * obs_dim / 1024), n_members), 256 threads: four consecutive floats per thread (one
//                         float4 when the member's run is 16-byte aligned), shift / scale staged in LDS.
//
// No atomics, no hand-off between workgroups: the same inputs give the same bits.  A unit of its own: adding kernels to an
// existing unit moves the old kernels' schedules, and tests/test_ppo_shapes.py pins those.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcc_policy.h"

namespace {

constexpr int kObsThreads = 256;
constexpr int kObsMaxDim = 128;
constexpr int kObsMaxMembers = 1024;
constexpr int kObsRowsPerLane = 64;    // rows a row lane sums in a chunk of the default size
constexpr int kObsMaxChunks = 2048;    // chunks of a member at the most: larger members get longer chunks

// How a member's n = T * n_m rows are cut: log2 of P, the chunk's rows (a multiple of the row lanes 256 / P) and their number.
struct ObsCut {
    int log2p;
    int64_t n, chunk;
    int chunks;
};

bool obs_cut(int T, int64_t n_m, int D, ObsCut *c) {
    if (T < 1 || n_m < 1 || D < 1 || D > kObsMaxDim || n_m > INT64_MAX / T) return false;
    int lg = 0;
    while ((1 << lg) < D) lg++;
    const int64_t R = kObsThreads >> lg, n = (int64_t)T * n_m;
    int64_t chunk = R * kObsRowsPerLane;
    if ((n + chunk - 1) / chunk > kObsMaxChunks) chunk = ((n + kObsMaxChunks - 1) / kObsMaxChunks + R - 1) / R * R;
    c->log2p = lg;
    c->n = n;
    c->chunk = chunk;
    c->chunks = (int)((n + chunk - 1) / chunk);
    return true;
}

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

__global__ __launch_bounds__(kObsThreads) void obs_moments_kernel(const float *__restrict__ obs, int64_t n_envs, int64_t n_m, int D,
                                                                  int log2p, int64_t n, int64_t chunk, double *__restrict__ scratch) {
    __shared__ double s_sum[4][kObsMaxDim], s_sq[4][kObsMaxDim];
    const int tid = threadIdx.x, P = 1 << log2p, R = kObsThreads >> log2p;
    const int f = tid & (P - 1), r = tid >> log2p;
    const int64_t start = (int64_t)blockIdx.x * chunk, end = start + chunk < n ? start + chunk : n;
    const float *base = obs + (int64_t)blockIdx.y * n_m * D;   // the member's run of row 0
    const int64_t row_stride = n_envs * D;
    int64_t t = start / n_m, e_lo = start % n_m;
    double s = 0.0, q = 0.0, k = 0.0;
    if (f < D) {
        k = (double)base[t * row_stride + e_lo * D + f];
        for (int64_t j = start; j < end; t++, e_lo = 0) {
            // the chunk's rows of step t: [e_lo, e_lo + seg) of the member's n_m, one contiguous run of seg * D floats
            const int64_t left = n_m - e_lo, seg = left < end - j ? left : end - j;
            const float *p = base + t * row_stride + e_lo * D + f;
            int64_t i = r;
            for (; i + 7 * R < seg; i += 8 * R) {   // eight loads in flight, summed in row order
                float x[8];
#pragma unroll
                for (int u = 0; u < 8; u++) x[u] = p[(i + u * R) * D];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const double d = (double)x[u] - k;
                    s += d; q += d * d;
                }
            }
            for (; i < seg; i += R) {
                const double d = (double)p[i * D] - k;
                s += d; q += d * d;
            }
            j += seg;
        }
    }
    // the row lanes of one wavefront (P < 64: lanes f, f + P, ...), by xor-shuffles: every lane ends with the same sum
    for (int d = 32; d >= P; d >>= 1) {
        s += __shfl_xor(s, d);
        q += __shfl_xor(q, d);
    }
    // ... then the groups that are left: the 4 wavefronts (P <= 64), or the 2 row lanes of P = 128
    const int group = P <= 64 ? tid >> 6 : r, n_groups = P <= 64 ? 4 : R;
    if (f < D && (P >= 64 || (tid & 63) < P)) {
        s_sum[group][f] = s;
        s_sq[group][f] = q;
    }
    __syncthreads();
    if (tid < D) {   // (f = tid, r = 0: its k is the feature's)
        double ss = s_sum[0][tid], qq = s_sq[0][tid];
        for (int g = 1; g < n_groups; g++) {
            ss += s_sum[g][tid];
            qq += s_sq[g][tid];
        }
        const double cnt = (double)(end - start);
        const double m2 = qq - ss * ss / cnt;
        double *out = scratch + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * D;
        out[tid] = k + ss / cnt;
        out[D + tid] = m2 > 0.0 ? m2 : 0.0;   // (a sum of squared deviations: rounding must not make it negative)
    }
}

__global__ __launch_bounds__(kObsThreads) void obs_merge_kernel(const double *__restrict__ scratch, int chunks, int64_t n, int64_t chunk,
                                                                int D, int log2p, double *__restrict__ stats, int64_t stat_stride,
                                                                float *__restrict__ norm, double eps) {
    __shared__ double s_red[kObsThreads];
    const int tid = threadIdx.x, P = 1 << log2p, S = kObsThreads >> log2p;
    const int f = tid & (P - 1), sub = tid >> log2p;
    const double *part = scratch + (int64_t)blockIdx.x * chunks * 2 * D;
    const int per = (chunks + S - 1) / S;
    const int g0 = sub * per, g1 = f < D ? ((sub + 1) * per < chunks ? (sub + 1) * per : chunks) : 0;   // (an idle lane: no chunk)
    // the sum over a feature's sub-lanes, to all of them: a fixed tree in LDS.  Every thread calls it.
    auto feature_sum = [&](double v) {
        __syncthreads();   // (the last call's reads are done)
        s_red[tid] = v;
        __syncthreads();
        for (int half = S >> 1; half >= 1; half >>= 1) {
            if (sub < half) s_red[tid] += s_red[tid + (half << log2p)];
            __syncthreads();
        }
        return s_red[f];
    };
    // The batch's moments from the chunks' {count, mean, m2} in one pass in index order, no division per chunk: with d_g the
    // distance of chunk g's mean from chunk 0's, mean = k + sum(count_g d_g) / n and m2 = sum(m2_g) + sum(count_g d_g^2) -
    // sum(count_g d_g)^2 / n.  Four chunks' loads in flight: the pass waits for memory, not for arithmetic.
    const double k = f < D ? part[f] : 0.0;
    double a1 = 0.0, a2 = 0.0, a3 = 0.0;
    auto count_of = [&](int g) {
        const int64_t left = n - (int64_t)g * chunk;
        return (double)(left < chunk ? left : chunk);
    };
    int g = g0;
    for (; g + 3 < g1; g += 4) {
        double mu[4], mq[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            mu[u] = part[(int64_t)(g + u) * 2 * D + f];
            mq[u] = part[(int64_t)(g + u) * 2 * D + D + f];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const double c = count_of(g + u), d = mu[u] - k;
            a1 += c * d; a2 += c * (d * d); a3 += mq[u];
        }
    }
    for (; g < g1; g++) {
        const double c = count_of(g), d = part[(int64_t)g * 2 * D + f] - k;
        a1 += c * d; a2 += c * (d * d); a3 += part[(int64_t)g * 2 * D + D + f];
    }
    const double na = (double)n, s1 = feature_sum(a1), s2 = feature_sum(a2), s3 = feature_sum(a3);
    const double between = s2 - s1 * s1 / na;
    const double ma = k + s1 / na, qa = s3 + (between > 0.0 ? between : 0.0);
    double *row = stats + (int64_t)blockIdx.x * stat_stride;
    double cnt = tid < D ? row[0] : 0.0;
    __syncthreads();   // (every feature's thread has read the count before thread 0 writes it)
    if (tid < D) {     // (f = tid, sub = 0): the batch into the member's running row
        double mean = row[1 + tid], m2 = row[1 + D + tid];
        chan_merge(cnt, mean, m2, na, ma, qa);
        if (tid == 0) row[0] = cnt;
        row[1 + tid] = mean;
        row[1 + D + tid] = m2;
        if (norm) {
            float *nr = norm + (int64_t)blockIdx.x * 2 * D;
            nr[tid] = (float)mean;
            nr[D + tid] = (float)(1.0 / sqrt(m2 / cnt + eps));
        }
    }
}

__global__ __launch_bounds__(kObsThreads) void obs_normalise_kernel(const float *obs, int64_t run, int D, const float *__restrict__ norm,
                                                                    float clip, float *out, int vec_ok) {
    __shared__ float s_norm[2 * kObsMaxDim];
    const int tid = threadIdx.x;
    const float *nr = norm + (int64_t)blockIdx.y * 2 * D;
    for (int i = tid; i < 2 * D; i += kObsThreads) s_norm[i] = nr[i];
    __syncthreads();
    const int64_t member = (int64_t)blockIdx.y * run;                    // the member's run of n_m * D floats
    const int64_t e = ((int64_t)blockIdx.x * kObsThreads + tid) * 4;
    if (e >= run) return;
    int d = (int)(e % D);
    float x[4];
    const int cnt = run - e < 4 ? (int)(run - e) : 4;
    const bool vec = vec_ok && cnt == 4;
    if (vec) {
        const float4 v = *reinterpret_cast<const float4 *>(obs + member + e);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
        for (int i = 0; i < 4; i++) x[i] = i < cnt ? obs[member + e + i] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        x[i] = fminf(fmaxf((x[i] - s_norm[d]) * s_norm[D + d], -clip), clip);
        d = d + 1 == D ? 0 : d + 1;
    }
    if (vec) {
        *reinterpret_cast<float4 *>(out + member + e) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
        for (int i = 0; i < cnt; i++) out[member + e + i] = x[i];
    }
}

bool obs_domain(int64_t n_envs, int obs_dim, int n_members) {
    return obs_dim >= 1 && obs_dim <= kObsMaxDim && n_members >= 1 && n_members <= kObsMaxMembers && n_envs >= 1 &&
           n_envs % n_members == 0;
}

}  // namespace

extern "C" int pcc_obs_stats_scratch_doubles(int T, int64_t n_envs, int obs_dim, int n_members) {
    ObsCut c;
    if (!obs_domain(n_envs, obs_dim, n_members) || !obs_cut(T, n_envs / n_members, obs_dim, &c)) return -1;
    const int64_t doubles = (int64_t)n_members * c.chunks * 2 * obs_dim;   // (at most 1024 * 2048 * 256 = 2^29)
    return doubles > 0x7fffffff ? -1 : (int)doubles;
}

extern "C" int pcc_obs_stats_update_pop(const float *obs, int T, int64_t n_envs, int obs_dim, int n_members, double *stats,
                                        int64_t stat_stride, float *norm, double eps, double *scratch, void *stream) {
    // (every refusal comes before any HIP call: a host without a device gives the same answers)
    ObsCut c;
    if (!obs || !stats || !scratch) return -1;
    if (!obs_domain(n_envs, obs_dim, n_members) || !obs_cut(T, n_envs / n_members, obs_dim, &c)) return -1;
    if (stat_stride < 1 + 2 * (int64_t)obs_dim || !(eps >= 0.0)) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(obs_moments_kernel, dim3((unsigned)c.chunks, (unsigned)n_members), dim3(kObsThreads), 0, st, obs, n_envs,
                       n_envs / n_members, obs_dim, c.log2p, c.n, c.chunk, scratch);
    if (hipGetLastError() != hipSuccess) return -3;
    hipLaunchKernelGGL(obs_merge_kernel, dim3((unsigned)n_members), dim3(kObsThreads), 0, st, scratch, c.chunks, c.n, c.chunk, obs_dim,
                       c.log2p, stats, stat_stride, norm, eps);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int pcc_obs_normalise_pop(const float *obs, int64_t n_envs, int obs_dim, int n_members, const float *norm, float clip,
                                     float *out, void *stream) {
    if (!obs || !norm || !out) return -1;
    if (!obs_domain(n_envs, obs_dim, n_members) || !(clip > 0.0f)) return -1;
    const int64_t n_m = n_envs / n_members;
    if (n_m > INT64_MAX / obs_dim / n_members) return -1;
    const int64_t run = n_m * obs_dim, blocks = (run + 4 * kObsThreads - 1) / (4 * kObsThreads);
    if (blocks > 0x7fffffff) return -1;
    // float4 when every member's run starts on 16 bytes; else float by float
    const int vec_ok = run % 4 == 0 && ((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
    hipLaunchKernelGGL(obs_normalise_kernel, dim3((unsigned)blocks, (unsigned)n_members), dim3(kObsThreads), 0,
                       static_cast<hipStream_t>(stream), obs, run, obs_dim, norm, clip, out, vec_ok);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// The stand-alone forms: a population of one (no twin kernels).
extern "C" int pcc_obs_stats_update(const float *obs, int T, int64_t n_envs, int obs_dim, double *stats, float *norm, double eps,
                                    double *scratch, void *stream) {
    return pcc_obs_stats_update_pop(obs, T, n_envs, obs_dim, 1, stats, 1 + 2 * (int64_t)obs_dim, norm, eps, scratch, stream);
}

extern "C" int pcc_obs_normalise(const float *obs, int64_t n_envs, int obs_dim, const float *norm, float clip, float *out,
                                 void *stream) {
    return pcc_obs_normalise_pop(obs, n_envs, obs_dim, 1, norm, clip, out, stream);
}
