// pcc_streams.hip -- keyed random streams of a learner and the standardisation of its advantages (include/pcc_policy.h:
// pcc_rollout_noise_pop, pcc_sample_order_pop, pcc_adv_standardise_pop and their stand-alone forms): what a
// PPO iteration draws -- the rollout's standard normals, every epoch's minibatch order -- as pure functions of (the learner's 64-bit
// key, iteration, step or epoch, the learner's LOCAL sample index), and (a - mean) / (std + 1e-8) per member in float64.
//
//   rollout_noise_kernel   grid (ceil(ceil(n_m / 4) / 256), n_members, min(T, 65535)), 256 threads: thread = one Philox block = four
//                          consecutive local envs 4 q .. 4 q + 3 of the member, rows blockIdx.z, + gridDim.z, ...  Two Box-Muller
//                          pairs in float64 per block, one float4 store when every member's run of every row is 16-byte aligned.
//   sample_order_kernel    grid (min(ceil(n / 256), 65536), n_members), 256 threads, positions i = thread, + grid, ...: the round keys
//                          from one Philox block per thread, then the 6-round Feistel network on 2 h bits, walked until the value is
//                          below n.  No sort, no communication: every position on its own.
//   adv_sum_kernel<P>      grid (G, n_members), 256 threads, G = ceil(n_m / 256): lane = local env, a member is cut into workgroups
//                          exactly as a launch over the member alone.  P = 0: the lane adds its T values in step order; P = 1: every
//                          workgroup first totals pass 0's partials of its member (member_total: the same order in every workgroup,
//                          so all of them hold the same mean) and the lane adds (a - mean)^2.  A wavefront's lanes in a down-shuffle
//                          tree, the four wavefronts in index order, the workgroup's sum to scratch[P][member][workgroup].
//   adv_apply_kernel       grid (G, n_members, min(T, 65535)): every workgroup totals pass 1's partials, then lane = local env
//                          writes float32((a - mean) / (sqrt(var) + 1e-8)) for its rows.
//
// No atomics, no hand-off between workgroups inside a launch, no synchronise: the same inputs give the same bits.  A unit of its own
// (see pcc_pbt.hip: adding kernels to an existing unit moves the old kernels' schedules).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcc_dev.h"   // philox4x32_10: the simulator's, not another copy
#include "pcc_policy.h"

namespace {

constexpr int kStrThreads = 256;
constexpr int kStrMaxMembers = 1024;
constexpr int kStrUnroll = 8;                 // rows whose loads are in flight together
constexpr uint32_t kTagNoise = 0x4E4F4953u;   // "NOIS": counter word 3 of the rollout's blocks
constexpr uint32_t kTagOrder = 0x4F524452u;   // "ORDR": ... of the blocks the round keys come from
constexpr int kFeistelRounds = 6;

// One Box-Muller pair from two words: u1 = (a + 1) / 2^32 in (0, 1], the angle 2 pi b / 2^32 = pi * (b / 2^31); float64 throughout,
// rounded to float32 once.
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float &z0, float &z1) {
    const double u1 = ((double)a + 1.0) * (1.0 / 4294967296.0);
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi((double)b * (1.0 / 2147483648.0), &s, &c);
    z0 = (float)(r * c);
    z1 = (float)(r * s);
}

__global__ __launch_bounds__(kStrThreads) void rollout_noise_kernel(float *__restrict__ noise, uint32_t *__restrict__ words, int T,
                                                                    int64_t n_envs, int64_t n_m, const uint64_t *__restrict__ keys,
                                                                    uint64_t key1, uint32_t iteration, int vec_ok) {
    const int64_t q = (int64_t)blockIdx.x * kStrThreads + threadIdx.x;   // the block: local envs 4 q .. 4 q + 3
    const int64_t e = 4 * q;
    if (e >= n_m) return;
    const uint64_t key = keys ? keys[blockIdx.y] : key1;
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    const int cnt = n_m - e < 4 ? (int)(n_m - e) : 4;
    const bool vec = vec_ok && cnt == 4;
    const int64_t col = (int64_t)blockIdx.y * n_m + e;
    for (int t = blockIdx.z; t < T; t += gridDim.z) {
        uint32_t w[4];
        philox4x32_10((uint32_t)q, (uint32_t)t, iteration, kTagNoise, k0, k1, w);
        float z[4];
        box_muller(w[0], w[1], z[0], z[1]);
        box_muller(w[2], w[3], z[2], z[3]);
        const int64_t at = (int64_t)t * n_envs + col;
        if (vec) {
            *reinterpret_cast<float4 *>(noise + at) = make_float4(z[0], z[1], z[2], z[3]);
            if (words) *reinterpret_cast<uint4 *>(words + at) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int j = 0; j < cnt; j++) {
                noise[at + j] = z[j];
                if (words) words[at + j] = w[j];
            }
        }
    }
}

// murmur3's 32-bit finaliser: a bijection of the 32-bit words with full avalanche
__device__ __forceinline__ uint32_t fmix32(uint32_t v) {
    v ^= v >> 16; v *= 0x85EBCA6Bu;
    v ^= v >> 13; v *= 0xC2B2AE35u;
    v ^= v >> 16;
    return v;
}

// the balanced Feistel network on 2 h bits (h <= 32): a bijection of [0, 4^h) whatever the round function is
__device__ __forceinline__ uint64_t feistel(uint64_t x, int h, uint32_t mask, const uint32_t (&rk)[kFeistelRounds]) {
    uint32_t L = (uint32_t)(x >> h), R = (uint32_t)x & mask;
#pragma unroll
    for (int r = 0; r < kFeistelRounds; r++) {
        const uint32_t f = fmix32(R + rk[r]) & mask;
        const uint32_t nl = R;
        R = L ^ f;
        L = nl;
    }
    return ((uint64_t)L << h) | (uint64_t)R;
}

__global__ __launch_bounds__(kStrThreads) void sample_order_kernel(int64_t *__restrict__ perm, int64_t perm_stride, int64_t n,
                                                                   int64_t n_envs, int64_t n_m, int h, const uint64_t *__restrict__ keys,
                                                                   uint64_t key1, uint32_t iteration, uint32_t epoch) {
    const uint64_t key = keys ? keys[blockIdx.y] : key1;
    uint32_t w[4], rk[kFeistelRounds];
    philox4x32_10(epoch, 0u, iteration, kTagOrder, (uint32_t)key, (uint32_t)(key >> 32), w);
#pragma unroll
    for (int r = 0; r < kFeistelRounds; r++) rk[r] = w[r & 3] + (uint32_t)r * 0x9E3779B9u;
    const uint32_t mask = h >= 32 ? 0xFFFFFFFFu : (1u << h) - 1u;
    const int64_t base = (int64_t)blockIdx.y * n_m;
    int64_t *row = perm + (int64_t)blockIdx.y * perm_stride;
    const bool narrow = n <= 0xFFFFFFFFll;   // (the same for every thread: the division in 32 bits)
    for (int64_t i = (int64_t)blockIdx.x * kStrThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kStrThreads) {
        // the walk follows the cycle of i under a permutation of [0, 4^h): it comes back to i, which is below n, so it ends
        uint64_t x = (uint64_t)i;
        do {
            x = feistel(x, h, mask, rk);
        } while (x >= (uint64_t)n);
        int64_t t, e;
        if (narrow) {
            const uint32_t tq = (uint32_t)x / (uint32_t)n_m;
            t = tq;
            e = (uint32_t)x - tq * (uint32_t)n_m;
        } else {
            t = (int64_t)(x / (uint64_t)n_m);
            e = (int64_t)x - t * n_m;
        }
        row[i] = t * n_envs + base + e;
    }
}

// The sum of a member's `groups` partials, to every thread; all 256 threads call it.  Sub-lane tid adds the partials [tid * per,
// tid * per + per), per = ceil(groups / 256), in index order from 0.0; then the tree x[j] += x[j + s] for j < s, s = 128, ..., 1.
__device__ __forceinline__ double member_total(const double *__restrict__ part, int groups, double *s_red) {
    const int tid = threadIdx.x;
    const int per = (groups + kStrThreads - 1) / kStrThreads;
    const int g0 = tid * per < groups ? tid * per : groups, g1 = g0 + per < groups ? g0 + per : groups;
    double a = 0.0;
    for (int g = g0; g < g1; g++) a += part[g];
    s_red[tid] = a;
    __syncthreads();
    for (int half = kStrThreads >> 1; half >= 1; half >>= 1) {
        if (tid < half) s_red[tid] += s_red[tid + half];
        __syncthreads();
    }
    const double total = s_red[0];
    __syncthreads();
    return total;
}

template <int PASS>
__global__ __launch_bounds__(kStrThreads) void adv_sum_kernel(const float *__restrict__ adv, int T, int64_t n_envs, int64_t n_m,
                                                              double *__restrict__ scratch, double *__restrict__ moments) {
    __shared__ double s_red[kStrThreads];
    __shared__ double s_wave[kStrThreads / 64];
    const int tid = threadIdx.x, groups = gridDim.x;
    const int64_t local = (int64_t)blockIdx.x * kStrThreads + tid;
    double mean = 0.0;
    if (PASS == 1) {
        const double total = member_total(scratch + (int64_t)blockIdx.y * groups, groups, s_red);
        mean = total / ((double)T * (double)n_m);
        if (blockIdx.x == 0 && tid == 0) moments[2 * blockIdx.y] = mean;
    }
    double s = 0.0;
    if (local < n_m) {
        const float *p = adv + (int64_t)blockIdx.y * n_m + local;
        auto term = [&](float a) {
            if (PASS == 0) {
                s += (double)a;
            } else {
                const double d = (double)a - mean;
                s += d * d;
            }
        };
        int t = 0;
        for (; t + kStrUnroll <= T; t += kStrUnroll) {
            float a[kStrUnroll];
#pragma unroll
            for (int u = 0; u < kStrUnroll; u++) a[u] = p[(int64_t)(t + u) * n_envs];
#pragma unroll
            for (int u = 0; u < kStrUnroll; u++) term(a[u]);
        }
        for (; t < T; t++) term(p[(int64_t)t * n_envs]);
    }
    // the wavefront's lanes in a down-shuffle tree (lane 0 ends with the wavefront's sum), then the 4 wavefronts in index order
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
    if ((tid & 63) == 0) s_wave[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kStrThreads / 64; w++) s += s_wave[w];
        scratch[((int64_t)PASS * gridDim.y + blockIdx.y) * groups + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kStrThreads) void adv_apply_kernel(const float *adv, int T, int64_t n_envs, int64_t n_m,
                                                                const double *__restrict__ scratch, double *__restrict__ moments,
                                                                float *out) {
    __shared__ double s_red[kStrThreads];
    const int groups = gridDim.x;
    const double total = member_total(scratch + ((int64_t)gridDim.y + blockIdx.y) * groups, groups, s_red);
    const double var = total / ((double)T * (double)n_m - 1.0);   // (one sample: 0 / 0, NaN, as torch's std)
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) moments[2 * blockIdx.y + 1] = var;
    const int64_t local = (int64_t)blockIdx.x * kStrThreads + threadIdx.x;
    if (local >= n_m) return;
    const double mean = moments[2 * blockIdx.y];   // (pass 1's launch wrote it)
    const double denom = sqrt(var) + 1e-8;
    const int64_t col = (int64_t)blockIdx.y * n_m + local;
    for (int t = blockIdx.z; t < T; t += gridDim.z) {
        const int64_t at = (int64_t)t * n_envs + col;
        out[at] = (float)(((double)adv[at] - mean) / denom);
    }
}

// the member's workgroups of the sums; -1 outside the domain (no index of the kernels overflows inside it)
int64_t str_groups(int T, int64_t n_envs, int n_members) {
    if (T < 1 || n_envs < 1 || n_members < 1 || n_members > kStrMaxMembers || n_envs % n_members != 0) return -1;
    if (n_envs / n_members > 0x7fffffffll) return -1;                       // (a local env index and its block fit 32 bits)
    if (n_envs > INT64_MAX / (int64_t)sizeof(double) / T) return -1;
    const int64_t groups = (n_envs / n_members + kStrThreads - 1) / kStrThreads;
    if (groups > 0x7fffffff / (2 * (int64_t)n_members)) return -1;
    return groups;
}

int rollout_noise(float *noise, uint32_t *words, int T, int64_t n_envs, int n_members, const uint64_t *keys, uint64_t key,
                  uint32_t iteration, void *stream) {
    // (every refusal comes before any HIP call: a host without a device gives the same answers)
    if (!noise || str_groups(T, n_envs, n_members) < 0) return -1;
    const int64_t n_m = n_envs / n_members, blocks = ((n_m + 3) / 4 + kStrThreads - 1) / kStrThreads;
    uintptr_t align = reinterpret_cast<uintptr_t>(noise) | reinterpret_cast<uintptr_t>(words);
    const int vec_ok = n_m % 4 == 0 && (align & 15u) == 0;
    hipLaunchKernelGGL(rollout_noise_kernel, dim3((unsigned)blocks, (unsigned)n_members, (unsigned)(T < 65535 ? T : 65535)),
                       dim3(kStrThreads), 0, static_cast<hipStream_t>(stream), noise, words, T, n_envs, n_m, keys, key, iteration, vec_ok);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int sample_order(int64_t *perm, int64_t perm_stride, int T, int64_t n_envs, int n_members, const uint64_t *keys, uint64_t key,
                 uint32_t iteration, uint32_t epoch, void *stream) {
    if (!perm || str_groups(T, n_envs, n_members) < 0) return -1;
    const int64_t n_m = n_envs / n_members, n = (int64_t)T * n_m;
    if (perm_stride < 0) perm_stride = n;   // (the stand-alone form: one row, exactly n long)
    if (perm_stride < n) return -1;
    int h = 0;   // the smallest even-bit domain 4^h >= n
    while (h < 31 && ((int64_t)1 << (2 * h)) < n) h++;
    int64_t blocks = (n + kStrThreads - 1) / kStrThreads;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(sample_order_kernel, dim3((unsigned)blocks, (unsigned)n_members), dim3(kStrThreads), 0,
                       static_cast<hipStream_t>(stream), perm, perm_stride, n, n_envs, n_m, h, keys, key, iteration, epoch);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

extern "C" int pcc_rollout_noise_pop(float *noise_out, uint32_t *words_out, int T, int64_t n_envs, int n_members, const uint64_t *keys,
                                     uint32_t iteration, void *stream) {
    if (!keys) return -1;
    return rollout_noise(noise_out, words_out, T, n_envs, n_members, keys, 0, iteration, stream);
}

extern "C" int pcc_sample_order_pop(int64_t *perm_out, int64_t perm_stride, int T, int64_t n_envs, int n_members, const uint64_t *keys,
                                    uint32_t iteration, uint32_t epoch, void *stream) {
    if (!keys || perm_stride < 0) return -1;
    return sample_order(perm_out, perm_stride, T, n_envs, n_members, keys, 0, iteration, epoch, stream);
}

extern "C" int pcc_adv_standardise_scratch_doubles(int T, int64_t n_envs, int n_members) {
    const int64_t groups = str_groups(T, n_envs, n_members);
    return groups < 0 ? -1 : (int)(2 * groups * n_members);
}

extern "C" int pcc_adv_standardise_pop(const float *adv, int T, int64_t n_envs, int n_members, double *scratch, double *moments_out,
                                       float *out, void *stream) {
    if (!adv || !scratch || !moments_out || !out) return -1;
    const int64_t groups = str_groups(T, n_envs, n_members);
    if (groups < 0) return -1;
    const int64_t n_m = n_envs / n_members;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)groups, (unsigned)n_members);
    hipLaunchKernelGGL(adv_sum_kernel<0>, grid, dim3(kStrThreads), 0, st, adv, T, n_envs, n_m, scratch, moments_out);
    if (hipGetLastError() != hipSuccess) return -3;
    hipLaunchKernelGGL(adv_sum_kernel<1>, grid, dim3(kStrThreads), 0, st, adv, T, n_envs, n_m, scratch, moments_out);
    if (hipGetLastError() != hipSuccess) return -3;
    hipLaunchKernelGGL(adv_apply_kernel, dim3((unsigned)groups, (unsigned)n_members, (unsigned)(T < 65535 ? T : 65535)), dim3(kStrThreads),
                       0, st, adv, T, n_envs, n_m, scratch, moments_out, out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// The stand-alone forms: a population of one (no twin kernels); the key comes as an argument, not from keys.
extern "C" int pcc_rollout_noise(float *noise_out, uint32_t *words_out, int T, int64_t n_envs, uint64_t key, uint32_t iteration,
                                 void *stream) {
    return rollout_noise(noise_out, words_out, T, n_envs, 1, nullptr, key, iteration, stream);
}

extern "C" int pcc_sample_order(int64_t *perm_out, int T, int64_t n_envs, uint64_t key, uint32_t iteration, uint32_t epoch,
                                void *stream) {
    return sample_order(perm_out, -1, T, n_envs, 1, nullptr, key, iteration, epoch, stream);
}

extern "C" int pcc_adv_standardise(const float *adv, int T, int64_t n_envs, double *scratch, double *moments_out, float *out,
                                   void *stream) {
    return pcc_adv_standardise_pop(adv, T, n_envs, 1, scratch, moments_out, out, stream);
}
