// pcc_mlp_tiles.h -- the PPO caller's two kernels for ANY policy of the supported domain (one sender, two tanh hidden layers,
// 1 <= obs_dim <= 128, 1 <= h1, h2 <= 64): the tiled generalisation of ppo_grad_mfma_kernel (pcc_ppo.hip) and of the policy
// forward (pcc_policy.hip); the parameter block's layout (PolicyLayout), tanh_fast, wave_sum and the Gaussian head are
// pcc_policy_dev.h's, shared with those.  obs_dim, h1, h2 are run-time values; a kernel is instantiated per TILE CLASS <DP, H1P, H2P>, the
// sizes rounded up (DP in {32, 64, 128}; (H1P, H2P) in {(32, 32), (64, 32), (64, 64)}), and everything between the real and the
// padded size is zero: padded weights, biases and W3 entries are 0, so a padded unit is tanh_fast(0) = 0 exactly (exp(0) = 1,
// rcp(2) = 0.5) and carries no gradient; padded rows / columns of dW are never stored.
//
// Layout.  A wavefront owns tiles of 32 samples.  Every contraction is v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf
// chain): operands come from LDS -- the CURRENT network's weights once per workgroup (rows padded to an odd stride: W1[unit][k]
// as a B operand is read down a column), the tile's activations sample-major in the wavefront's own buffers -- and results land
// in the C layout (lane & 31 = output column, the 16 registers = rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)).  Contractions over
// features / units (forward, dh1) loop at run time to the REAL size (rounded up to the MFMA's k = 2); only the output side is
// padded to blocks of 32.  The weight gradients dW = dZ^T X contract over the tile's 32 samples into accumulators that stay in
// registers over all tiles of the wavefront: at the largest class (128; 64, 64) dW1 is 128 and dW2 64 registers, which is why
// the gradient kernel runs ONE network per pass (policy, then value: the observation rows are gathered twice) -- both networks'
// accumulators (384) plus a tile's activations do not fit the 512 registers of a wavefront.
// LDS at (128; 64, 64): weights 12 612 floats + 8 416 per wavefront; 160 KiB hold three wavefronts (four in the other classes).
// Both kernels serve the stand-alone and the population entry points: the member is one more grid dimension (one member, zero
// strides and hyper == NULL in a stand-alone call), and the translation units pcc_mlp_tiles_d32/d64/d128.hip hold all of them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcc_policy_dev.h"

namespace pcc_tiles {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWave = 64;
constexpr int kTile = 32;           // samples per tile
constexpr int kMaxGradBlocks = 256; // one workgroup per CU (LDS)

using pcc::tanh_fast;
using pcc::wave_sum;
using Shape = pcc::PolicyLayout;   // the real sizes and the offsets inside one network's block of the parameter vector

template <int DP, int H1P, int H2P>
struct Cls {
    static_assert((DP == 32 || DP == 64 || DP == 128) && (H1P == 32 || H1P == 64) && (H2P == 32 || H2P == 64) && H2P <= H1P, "tile class");
    static constexpr int SX = DP + 1, S1 = H1P + 1, S2 = H2P + 1;                    // odd row strides: conflict-free both ways
    // the workgroup's weight area (padded layout), floats
    static constexpr int W1 = 0, W2 = W1 + H1P * SX, B1 = W2 + H2P * S1, B2 = B1 + H1P, W3 = B2 + H2P, B3 = W3 + H2P, NW = (B3 + 1 + 3) / 4 * 4;
    // a wavefront's buffers: x [32][SX] | h1 [32][S1] | z [32][S1] (h2, dz2 with stride S2; then dz1 with stride S1) | d out [32]
    static constexpr int XS = 0, H1S = XS + kTile * SX, ZS = H1S + kTile * S1, SC = ZS + kTile * S1, NWAVE = SC + kTile;
    static constexpr int kWaves = (DP == 128 && H1P == 64) ? 3 : 4;
    static constexpr int kLds = NW + kWaves * NWAVE;
    static_assert(kLds * 4 <= 160 * 1024, "LDS of a CU");
    static_assert(NW >= H1P * DP + H1P + H2P * H1P + 2 * H2P + 1, "the block's gradient is reduced in the weight area");
};

__device__ __forceinline__ uint32_t c_row(int r, uint32_t lane) { return (uint32_t)(r & 3) + 8u * (uint32_t)(r >> 2) + 4u * (lane >> 5); }

// LDS written by some lanes of a wavefront and read by others of it (LDS operations of a wavefront complete in order)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one network's parameters -> the workgroup's weight area, zero in every padded place (all threads; the caller synchronises)
template <int DP, int H1P, int H2P>
__device__ __forceinline__ void load_weights(float *Ws, const float *__restrict__ p, const Shape &s, int tid, int nthreads) {
    using C = Cls<DP, H1P, H2P>;
#pragma unroll 8   // (eight independent loads in flight: the staging is a chain of global-load latencies otherwise)
    for (int e = tid; e < H1P * C::SX; e += nthreads) {
        const int i = e / C::SX, k = e % C::SX;
        Ws[C::W1 + e] = (i < s.h1 && k < s.D) ? p[s.W1 + i * s.D + k] : 0.0f;
    }
#pragma unroll 8
    for (int e = tid; e < H2P * C::S1; e += nthreads) {
        const int j = e / C::S1, k = e % C::S1;
        Ws[C::W2 + e] = (j < s.h2 && k < s.h1) ? p[s.W2 + j * s.h1 + k] : 0.0f;
    }
    for (int e = tid; e < H1P; e += nthreads) Ws[C::B1 + e] = e < s.h1 ? p[s.B1 + e] : 0.0f;
    for (int e = tid; e < H2P; e += nthreads) {
        Ws[C::B2 + e] = e < s.h2 ? p[s.B2 + e] : 0.0f;
        Ws[C::W3 + e] = e < s.h2 ? p[s.W3 + e] : 0.0f;
    }
    if (tid == 0) Ws[C::B3] = p[s.B3];
}

// the tile's observation rows, sample-major with zeros beyond D and for samples that do not exist: idx = the row of sample
// (lane & 31), < 0 for none.  Element e = 64 it + lane of the [32][DP] tile: consecutive lanes read consecutive floats of a row.
template <int DP>
__device__ __forceinline__ void gather_tile(float *Xs, const float *__restrict__ obs, int64_t idx, int D, uint32_t lane) {
    constexpr int SX = DP + 1;
#pragma unroll 4
    for (int it = 0; it < kTile * DP / kWave; it++) {
        const uint32_t e = (uint32_t)it * kWave + lane, s = e / DP, c = e % DP;
        const int64_t row = __shfl(idx, (int)s, kWave);
        Xs[s * SX + c] = (row >= 0 && (int)c < D) ? obs[row * D + c] : 0.0f;
    }
}

// forward of the network in the weight area over the tile in Xs: h1 / h2 in the C layout (block u = units 32 u ..), H1s = h1
// sample-major, Zs = h2 sample-major (stride S2); returns the network's output for sample (lane & 31) (both lane halves).
template <int DP, int H1P, int H2P>
__device__ __forceinline__ float tile_forward(const float *Ws, const float *Xs, float *H1s, float *Zs, uint32_t lane, const Shape &s,
                                              f32x16 (&h1)[H1P / 32], f32x16 (&h2)[H2P / 32]) {
    using C = Cls<DP, H1P, H2P>;
    const uint32_t col = lane & 31u, hi = lane >> 5;
#pragma unroll
    for (int u = 0; u < H1P / 32; u++) {
        const float b = Ws[C::B1 + 32 * u + col];
#pragma unroll
        for (int r = 0; r < 16; r++) h1[u][r] = b;
    }
    {
        const float *xa = Xs + col * C::SX + hi, *wb = Ws + C::W1 + col * C::SX + hi;
        const int kD = (s.D + 1) >> 1;
#pragma unroll 4
        for (int t = 0; t < kD; t++) {
            const float a = xa[2 * t];
#pragma unroll
            for (int u = 0; u < H1P / 32; u++) h1[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb[32 * u * C::SX + 2 * t], h1[u], 0, 0, 0);
        }
    }
#pragma unroll
    for (int u = 0; u < H1P / 32; u++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            h1[u][r] = tanh_fast(h1[u][r]);
            H1s[c_row(r, lane) * C::S1 + 32 * u + col] = h1[u][r];
        }
    }
    wave_sync();
#pragma unroll
    for (int u = 0; u < H2P / 32; u++) {
        const float b = Ws[C::B2 + 32 * u + col];
#pragma unroll
        for (int r = 0; r < 16; r++) h2[u][r] = b;
    }
    {
        const float *ha = H1s + col * C::S1 + hi, *wb = Ws + C::W2 + col * C::S1 + hi;
        const int kH = (s.h1 + 1) >> 1;
#pragma unroll 4
        for (int t = 0; t < kH; t++) {
            const float a = ha[2 * t];
#pragma unroll
            for (int u = 0; u < H2P / 32; u++) h2[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb[32 * u * C::S1 + 2 * t], h2[u], 0, 0, 0);
        }
    }
#pragma unroll
    for (int u = 0; u < H2P / 32; u++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            h2[u][r] = tanh_fast(h2[u][r]);
            Zs[c_row(r, lane) * C::S2 + 32 * u + col] = h2[u][r];
        }
    }
    wave_sync();
    // layer 3, lane = sample: each lane half an ordered fmaf chain over half of the units, the halves added
    float part = 0.0f;
    {
        const float *z = Zs + col * C::S2 + hi * (H2P / 2), *w3 = Ws + C::W3 + hi * (H2P / 2);
#pragma unroll
        for (int j = 0; j < H2P / 2; j++) part = fmaf(w3[j], z[j], part);
    }
    part += __shfl_xor(part, 32, kWave);
    wave_sync();   // (Zs is free for dz2)
    return part + Ws[C::B3];
}

template <int H1P, int H2P, int DP>
struct GradAcc {   // one network's gradient sums of a wavefront
    f32x16 w1[H1P / 32][DP / 32];   // dW1 block: rows = units (C layout), lane = feature
    f32x16 w2[H2P / 32][H1P / 32];  // dW2 block: rows = units j, lane = k
    float b1[H1P / 32], b2[H2P / 32], w3[H2P / 32];   // per-lane partial sums for unit 32 u + (lane & 31) (both lane halves count)
    float b3;                       // lane = sample (lanes below 32 count)
};

// backward over the tile given d loss / d output of sample (lane & 31) in `dout` (0 for samples that do not exist)
template <int DP, int H1P, int H2P>
__device__ __forceinline__ void tile_backward(const float *Ws, GradAcc<H1P, H2P, DP> &g, const float *Xs, const float *H1s, float *Zs, float *Sc,
                                              uint32_t lane, const Shape &s, const f32x16 (&h1)[H1P / 32], const f32x16 (&h2)[H2P / 32],
                                              float dout) {
    using C = Cls<DP, H1P, H2P>;
    const uint32_t col = lane & 31u, hi = lane >> 5;
    if (hi == 0u) { Sc[col] = dout; g.b3 += dout; }
    wave_sync();
    // ---- layer 3 and the pre-activation gradient of layer 2 (C layout), sample-major to LDS
    float d[16];
#pragma unroll
    for (int r = 0; r < 16; r++) d[r] = Sc[c_row(r, lane)];
#pragma unroll
    for (int u = 0; u < H2P / 32; u++) {
        const float w3 = Ws[C::W3 + 32 * u + col];
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float h = h2[u][r];
            const float dz2 = d[r] * w3 * (1.0f - h * h);
            g.w3[u] = fmaf(d[r], h, g.w3[u]);
            g.b2[u] += dz2;
            Zs[c_row(r, lane) * C::S2 + 32 * u + col] = dz2;
        }
    }
    wave_sync();
    // ---- dW2[j][k] += sum_s dz2[s][j] h1[s][k]   (A[i = j][k = s], B[k = s][col = k])
#pragma unroll
    for (int t = 0; t < kTile / 2; t++) {
        const uint32_t sm = 2u * t + hi;
        float b[H1P / 32];
#pragma unroll
        for (int v = 0; v < H1P / 32; v++) b[v] = H1s[sm * C::S1 + 32 * v + col];
#pragma unroll
        for (int u = 0; u < H2P / 32; u++) {
            const float a = Zs[sm * C::S2 + 32 * u + col];
#pragma unroll
            for (int v = 0; v < H1P / 32; v++) g.w2[u][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[v], g.w2[u][v], 0, 0, 0);
        }
    }
    // ---- dh1[s][k] = sum_j dz2[s][j] W2[j][k]; dz1 = dh1 (1 - h1^2)   (A[i = s][k = j], B[k = j][col = k])
    f32x16 dz1[H1P / 32];
#pragma unroll
    for (int v = 0; v < H1P / 32; v++)
#pragma unroll
        for (int r = 0; r < 16; r++) dz1[v][r] = 0.0f;
    {
        const float *za = Zs + col * C::S2 + hi, *wb = Ws + C::W2 + hi * C::S1 + col;
        const int kJ = (s.h2 + 1) >> 1;
#pragma unroll 4
        for (int t = 0; t < kJ; t++) {
            const float a = za[2 * t];
#pragma unroll
            for (int v = 0; v < H1P / 32; v++) dz1[v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb[2 * t * C::S1 + 32 * v], dz1[v], 0, 0, 0);
        }
    }
#pragma unroll
    for (int v = 0; v < H1P / 32; v++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            dz1[v][r] *= 1.0f - h1[v][r] * h1[v][r];
            g.b1[v] += dz1[v][r];
        }
    }
    wave_sync();   // (every read of dz2 is done: dz1 takes the buffer over, stride S1)
#pragma unroll
    for (int v = 0; v < H1P / 32; v++)
#pragma unroll
        for (int r = 0; r < 16; r++) Zs[c_row(r, lane) * C::S1 + 32 * v + col] = dz1[v][r];
    wave_sync();
    // ---- dW1[i][f] += sum_s dz1[s][i] x[s][f]   (A[i][k = s], B[k = s][col = f])
#pragma unroll
    for (int t = 0; t < kTile / 2; t++) {
        const uint32_t sm = 2u * t + hi;
        float b[DP / 32];
#pragma unroll
        for (int f = 0; f < DP / 32; f++) b[f] = Xs[sm * C::SX + 32 * f + col];
#pragma unroll
        for (int v = 0; v < H1P / 32; v++) {
            const float a = Zs[sm * C::S1 + 32 * v + col];
#pragma unroll
            for (int f = 0; f < DP / 32; f++) g.w1[v][f] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[f], g.w1[v][f], 0, 0, 0);
        }
    }
    wave_sync();   // (the next tile's gather overwrites Xs)
}

// a wavefront's sums added to the block's gradient of one network in `G` (the real layout of include/pcc_policy.h)
template <int DP, int H1P, int H2P>
__device__ __forceinline__ void acc_store(const GradAcc<H1P, H2P, DP> &g, float *G, const Shape &s, uint32_t lane) {
    auto put = [&](int idx, float v) { G[idx] += v; };
    const int col = (int)(lane & 31u);
#pragma unroll
    for (int v = 0; v < H1P / 32; v++)
#pragma unroll
        for (int f = 0; f < DP / 32; f++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int i = 32 * v + (int)c_row(r, lane), k = 32 * f + col;
                if (i < s.h1 && k < s.D) put(s.W1 + i * s.D + k, g.w1[v][f][r]);
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // (a few stores in flight, not 128: registers)
            }
#pragma unroll
    for (int u = 0; u < H2P / 32; u++)
#pragma unroll
        for (int v = 0; v < H1P / 32; v++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int j = 32 * u + (int)c_row(r, lane), k = 32 * v + col;
                if (j < s.h2 && k < s.h1) put(s.W2 + j * s.h1 + k, g.w2[u][v][r]);
                if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
    for (int v = 0; v < H1P / 32; v++) {
        const float b1 = g.b1[v] + __shfl_xor(g.b1[v], 32, kWave);
        if (lane < 32u && 32 * v + col < s.h1) put(s.B1 + 32 * v + col, b1);
    }
#pragma unroll
    for (int u = 0; u < H2P / 32; u++) {
        const float b2 = g.b2[u] + __shfl_xor(g.b2[u], 32, kWave), w3 = g.w3[u] + __shfl_xor(g.w3[u], 32, kWave);
        if (lane < 32u && 32 * u + col < s.h2) { put(s.B2 + 32 * u + col, b2); put(s.W3 + 32 * u + col, w3); }
    }
    const float b3 = wave_sum(g.b3);
    if (lane == 0u) put(s.B3, b3);
}

// ======================================================================================
// ppo_grad_tiled_kernel: pcc_ppo_minibatch_step's gradient for the shapes ppo_grad_mfma_kernel has no instantiation for.  The
// same objective, masks and statistics; pass 0 = the policy network (+ log_std, statistics 0 and 2), pass 1 = the value network
// (statistic 1).  Every workgroup writes ONE partial gradient (2 n_net + 1 parameters + 4 statistics): its wavefronts' sums are
// added in the weight area in wavefront order once the pass's tiles are done.  No atomics: deterministic.
// blockIdx.y = member of a population, as in ppo_grad_mfma_kernel (one member, hyper == NULL and perm_all possibly NULL in a
// stand-alone call): its permutation row, parameter block, clip (hyper[m][1]) and slice of the partial-gradient scratch.
// ======================================================================================
template <int DP, int H1P, int H2P>
__global__ __launch_bounds__((Cls<DP, H1P, H2P>::kWaves) * 64, 1) void ppo_grad_tiled_kernel(
    const float *__restrict__ obs, const float *__restrict__ act, const float *__restrict__ logp_old,
    const float *__restrict__ adv, const float *__restrict__ ret, const int64_t *__restrict__ perm_all, int64_t perm_stride,
    int64_t start, int64_t count, int D, int n_h1, int n_h2, const float *__restrict__ params_all, int64_t param_stride,
    const float *__restrict__ hyper, float clip_arg, float *__restrict__ partial_all, int64_t partial_stride) {
    const int64_t member = blockIdx.y;
    const int64_t *perm = perm_all ? perm_all + member * perm_stride : nullptr;
    const float *params = params_all + member * param_stride;
    float *partial = partial_all + member * partial_stride;
    float clip = hyper ? hyper[member * 8 + 1] : clip_arg;
    // (the member's pointers are made here, once, in scalar registers: left to the scheduler, (128; 64, 32) spills six vector registers)
    asm volatile("" : "+s"(perm), "+s"(params), "+s"(partial), "+s"(clip));
    using C = Cls<DP, H1P, H2P>;
    constexpr int kWaves = C::kWaves;
    __shared__ float lds[C::kLds];
    __shared__ float red[kWaves][4];
    const Shape s(D, n_h1, n_h2);
    const int n_params = s.n_params();
    const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave, col = lane & 31u;
    float *Ws = lds, *Xs = lds + C::NW + wv * C::NWAVE + C::XS, *H1s = lds + C::NW + wv * C::NWAVE + C::H1S;
    float *Zs = lds + C::NW + wv * C::NWAVE + C::ZS, *Sc = lds + C::NW + wv * C::NWAVE + C::SC;
    const float log_std = params[s.log_std()];
    const float inv_std = __expf(-log_std);
    const float inv_n = 1.0f / (float)count;
    const int64_t n_tiles = (count + kTile - 1) / kTile;
    float *out_p = partial + (int64_t)blockIdx.x * (n_params + 4);
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {
        load_weights<DP, H1P, H2P>(Ws, params + (pass ? s.vf() : 0), s, (int)threadIdx.x, kWaves * kWave);
        __syncthreads();
        GradAcc<H1P, H2P, DP> g;
#pragma unroll
        for (int v = 0; v < H1P / 32; v++) {
            g.b1[v] = 0.0f;
#pragma unroll
            for (int f = 0; f < DP / 32; f++)
#pragma unroll
                for (int r = 0; r < 16; r++) g.w1[v][f][r] = 0.0f;
        }
#pragma unroll
        for (int u = 0; u < H2P / 32; u++) {
            g.b2[u] = g.w3[u] = 0.0f;
#pragma unroll
            for (int v = 0; v < H1P / 32; v++)
#pragma unroll
                for (int r = 0; r < 16; r++) g.w2[u][v][r] = 0.0f;
        }
        g.b3 = 0.0f;
        float st0 = 0.0f, st1 = 0.0f, st2 = 0.0f;   // pass 0: d log_std, surrogate, clipped; pass 1: squared value error
#pragma unroll 1
        for (int64_t tile = (int64_t)blockIdx.x * kWaves + wv; tile < n_tiles; tile += (int64_t)gridDim.x * kWaves) {
            const int64_t k = tile * kTile + col;
            const bool valid = k < count;
            const int64_t idx = valid ? (perm ? perm[start + k] : start + k) : -1;
            gather_tile<DP>(Xs, obs, idx, D, lane);
            wave_sync();
            f32x16 h1[H1P / 32], h2[H2P / 32];
            const float out = tile_forward<DP, H1P, H2P>(Ws, Xs, H1s, Zs, lane, s, h1, h2);
            float dout = 0.0f;
            if (pass == 0) {   // log-probability of the taken action, clipped surrogate (ppo_grad_mfma_kernel's arithmetic: keep in step)
                const float a = valid ? act[idx] : 0.0f, lp_old = valid ? logp_old[idx] : 0.0f, ad = valid ? adv[idx] : 0.0f;
                const float z = (a - out) * inv_std;
                const float lp = pcc::gaussian_logp(z, log_std);
                const float ratio = __expf(lp - lp_old);
                const float lo = 1.0f - clip, hi = 1.0f + clip;
                const float rc = fminf(fmaxf(ratio, lo), hi);
                const float surr1 = ratio * ad, surr2 = rc * ad;
                const bool through = surr1 <= surr2;   // min picks the unclipped term (inside the range both are the same)
                const float dlp = (valid && through) ? -ad * ratio * inv_n : 0.0f;
                dout = dlp * z * inv_std;
                if (valid && lane < 32u) {   // (the two lane halves hold the same sample: one of them counts)
                    st0 += dlp * (z * z - 1.0f);
                    st1 += fminf(surr1, surr2);
                    st2 += (ratio < lo || ratio > hi) ? 1.0f : 0.0f;
                }
            } else {           // 0.5 * mean((v - ret)^2)
                const float err = valid ? out - ret[idx] : 0.0f;
                dout = err * inv_n;
                if (lane < 32u) st0 += err * err;
            }
            tile_backward<DP, H1P, H2P>(Ws, g, Xs, H1s, Zs, Sc, lane, s, h1, h2, dout);
        }
        // ---- the block's partial gradient of this network: every wavefront's sums into the weight area, one after the other
        {
            const float a = wave_sum(st0), b = wave_sum(st1), c = wave_sum(st2);
            if (lane == 0u) { red[wv][0] = a; red[wv][1] = b; red[wv][2] = c; }
        }
        __syncthreads();   // (every wavefront has read its last weights)
        for (int k = (int)threadIdx.x; k < s.N; k += kWaves * kWave) Ws[k] = 0.0f;
        __syncthreads();
        for (uint32_t w = 0; w < (uint32_t)kWaves; w++) {   // in wavefront order: a fixed order of additions
            if (wv == w) {
                uint32_t l = lane;
                asm volatile("" : "+v"(l));   // (the ~200 store addresses are computed here, not hoisted above the tile loop: registers)
                acc_store<DP, H1P, H2P>(g, Ws, s, l);
            }
            __syncthreads();
        }
        float *dst = out_p + (pass ? s.vf() : 0);
        for (int k = (int)threadIdx.x; k < s.N; k += kWaves * kWave) dst[k] = Ws[k];
        if (threadIdx.x == 0) {
            float a = red[0][0], b = red[0][1], c = red[0][2];
            for (int w = 1; w < kWaves; w++) { a += red[w][0]; b += red[w][1]; c += red[w][2]; }
            if (pass == 0) {
                out_p[s.log_std()] = a;
                out_p[n_params + 0] = b;
                out_p[n_params + 2] = c;
            } else {
                out_p[n_params + 1] = a;
                out_p[n_params + 3] = 0.0f;
            }
        }
        __syncthreads();   // (the weight area and `red` are free for the next pass)
    }
}

// ======================================================================================
// policy_act_tiled_kernel: pcc_policy_act for the shapes its older kernels refuse -- the forward above, blockIdx.y = network
// (0: pi -> mean, action, log-probability; 1: vf -> value) like policy_act_fixed_kernel.  A sample's result does not depend on
// where in a tile or batch it sits (each row of an MFMA result is that row's own fmaf chain).
// blockIdx.z = member of a population (one in a stand-alone call): n = the member's rows, which it sees with its parameter block
// through offset pointers -- tiles start at the member's first row, as in a stand-alone launch over them.
// ======================================================================================
template <int DP, int H1P, int H2P>
__global__ __launch_bounds__((Cls<DP, H1P, H2P>::kWaves) * 64, 1) void policy_act_tiled_kernel(
    const float *__restrict__ obs_all, int64_t n, int D, int n_h1, int n_h2, const float *__restrict__ params_all, int64_t param_stride,
    const float *__restrict__ noise_all, float *__restrict__ mean_all, float *__restrict__ act_all, float *__restrict__ logp_all,
    float *__restrict__ value_all) {
    const int64_t member = blockIdx.z, off = member * n;
    const float *__restrict__ obs = obs_all + off * D, *__restrict__ params = params_all + member * param_stride;
    const float *__restrict__ noise = noise_all ? noise_all + off : nullptr;
    float *__restrict__ mean_out = mean_all ? mean_all + off : nullptr, *__restrict__ act_out = act_all ? act_all + off : nullptr;
    float *__restrict__ logp_out = logp_all ? logp_all + off : nullptr, *__restrict__ value_out = value_all ? value_all + off : nullptr;
    using C = Cls<DP, H1P, H2P>;
    constexpr int kWaves = C::kWaves;
    __shared__ float lds[C::kLds];
    const Shape s(D, n_h1, n_h2);
    const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave, col = lane & 31u;
    float *Ws = lds, *Xs = lds + C::NW + wv * C::NWAVE + C::XS, *H1s = lds + C::NW + wv * C::NWAVE + C::H1S;
    float *Zs = lds + C::NW + wv * C::NWAVE + C::ZS;
    const int net = (int)blockIdx.y;
    load_weights<DP, H1P, H2P>(Ws, params + (net ? s.vf() : 0), s, (int)threadIdx.x, kWaves * kWave);
    __syncthreads();
    const float log_std = params[s.log_std()];
    const int64_t n_tiles = (n + kTile - 1) / kTile;
#pragma unroll 1
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wv; tile < n_tiles; tile += (int64_t)gridDim.x * kWaves) {
        const int64_t i = tile * kTile + col;
        const bool valid = i < n;
        gather_tile<DP>(Xs, obs, valid ? i : -1, D, lane);
        wave_sync();
        f32x16 h1[H1P / 32], h2[H2P / 32];
        const float out = tile_forward<DP, H1P, H2P>(Ws, Xs, H1s, Zs, lane, s, h1, h2);
        if (valid && lane < 32u) {
            if (net == 0) {
                const float eps = noise ? noise[i] : 0.0f;
                if (mean_out) mean_out[i] = out;
                if (act_out) act_out[i] = pcc::gaussian_act(out, log_std, eps);
                if (logp_out) logp_out[i] = pcc::gaussian_logp(eps, log_std);
            } else if (value_out) {
                value_out[i] = out;
            }
        }
    }
}

// ---- host side: one translation unit per DP (pcc_mlp_tiles_d*.hip) instantiates its three hidden classes.  The argument blocks
// serve the stand-alone entry points (n_members = 1, strides 0, hyper NULL) and the population's.
struct GradArgs {
    const float *obs, *act, *logp_old, *adv, *ret;
    const int64_t *perm;     // member 0's row (may be NULL: the samples in order)
    int64_t perm_stride, start, count;
    int D, h1, h2;
    const float *params;     // member 0's block
    int64_t param_stride;
    const float *hyper;      // [n_members][8] on the device, or NULL: `clip` below
    float clip;
    float *partial;          // member 0's slice of the scratch
    int64_t partial_stride;
    int n_members;
};
struct ActArgs {             // n = a member's rows; every row pointer is the whole batch's
    const float *obs;
    int64_t n;
    int D, h1, h2;
    const float *params;
    int64_t param_stride;
    int n_members;
    const float *noise;
    float *mean_out, *act_out, *logp_out, *value_out;
};

// one tile class's launch: the same name for both kernels, told apart by the argument block
template <int DP, int H1P, int H2P>
inline int launch_class(const GradArgs &a, hipStream_t st, int *blocks_out) {
    using C = Cls<DP, H1P, H2P>;
    const int64_t tiles = (a.count + kTile - 1) / kTile;
    int64_t blocks = (tiles + C::kWaves - 1) / C::kWaves;
    if (blocks > kMaxGradBlocks) blocks = kMaxGradBlocks;
    *blocks_out = (int)blocks;
    hipLaunchKernelGGL((ppo_grad_tiled_kernel<DP, H1P, H2P>), dim3((unsigned)blocks, (unsigned)a.n_members), dim3(C::kWaves * kWave), 0, st,
                       a.obs, a.act, a.logp_old, a.adv, a.ret, a.perm, a.perm_stride, a.start, a.count, a.D, a.h1, a.h2, a.params,
                       a.param_stride, a.hyper, a.clip, a.partial, a.partial_stride);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <int DP, int H1P, int H2P>
inline int launch_class(const ActArgs &a, hipStream_t st, int *) {
    using C = Cls<DP, H1P, H2P>;
    const int64_t tiles = (a.n + kTile - 1) / kTile;
    int64_t blocks = (tiles + C::kWaves - 1) / C::kWaves;
    if (blocks > 128) blocks = 128;   // (a workgroup stages the weights once and walks its tiles; 2 x 128 = one per CU)
    hipLaunchKernelGGL((policy_act_tiled_kernel<DP, H1P, H2P>), dim3((unsigned)blocks, 2, (unsigned)a.n_members), dim3(C::kWaves * kWave), 0,
                       st, a.obs, a.n, a.D, a.h1, a.h2, a.params, a.param_stride, a.noise, a.mean_out, a.act_out, a.logp_out, a.value_out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

// the hidden class of (h1, h2) at observation class DP, for either argument block
template <int DP, class Args>
inline int launch_d(const Args &a, hipStream_t st, int *blocks_out = nullptr) {
    if (a.h1 <= 32 && a.h2 <= 32) return launch_class<DP, 32, 32>(a, st, blocks_out);
    if (a.h2 <= 32) return launch_class<DP, 64, 32>(a, st, blocks_out);
    return launch_class<DP, 64, 64>(a, st, blocks_out);
}

// the domain both kernels cover (pcc_ppo_supported)
inline bool in_domain(int D, int h1, int h2) { return D >= 1 && D <= 128 && h1 >= 1 && h1 <= 64 && h2 >= 1 && h2 <= 64; }

// defined in pcc_mlp_tiles_d32.hip / _d64.hip / _d128.hip
int launch_grad_d32(const GradArgs &a, hipStream_t st, int *blocks_out);
int launch_grad_d64(const GradArgs &a, hipStream_t st, int *blocks_out);
int launch_grad_d128(const GradArgs &a, hipStream_t st, int *blocks_out);
int launch_act_d32(const ActArgs &a, hipStream_t st);
int launch_act_d64(const ActArgs &a, hipStream_t st);
int launch_act_d128(const ActArgs &a, hipStream_t st);

inline int launch_grad(const GradArgs &a, hipStream_t st, int *blocks_out) {
    if (!in_domain(a.D, a.h1, a.h2)) return -2;
    return a.D <= 32 ? launch_grad_d32(a, st, blocks_out) : a.D <= 64 ? launch_grad_d64(a, st, blocks_out) : launch_grad_d128(a, st, blocks_out);
}
inline int launch_act(const ActArgs &a, hipStream_t st) {
    if (!in_domain(a.D, a.h1, a.h2)) return -2;
    return a.D <= 32 ? launch_act_d32(a, st) : a.D <= 64 ? launch_act_d64(a, st) : launch_act_d128(a, st);
}

}  // namespace pcc_tiles
