// pcc_mlp_tiles_pop.h -- the tiled kernels of pcc_mlp_tiles.h for a population (include/pcc_policy.h: pcc_policy_act_pop,
// pcc_ppo_minibatch_step_pop): the member is one more grid dimension, and a workgroup of member m runs the stand-alone kernel's
// code on that member's rows, permutation, parameter block and scratch slice through offset pointers -- the same grid in x, the
// same tiles per wavefront, the same order of every sum, so the same bits as n_members stand-alone launches.
// The two bodies below are ppo_grad_tiled_kernel's and policy_act_tiled_kernel's, statement for statement, and are kept in step
// by hand (tests/test_population.py holds them against each other bit for bit): calling one shared body from the old kernels too
// was tried and moves their code (other schedules, other register counts), and so does instantiating the population kernels in
// the old kernels' translation units -- these are instantiated in units of their own (pcc_mlp_tiles_pop_d*.hip).
#pragma once
#include "pcc_mlp_tiles.h"

namespace pcc_tiles {

template <int DP, int H1P, int H2P>
__device__ __forceinline__ void ppo_grad_tiled_body(const float *__restrict__ obs, const float *__restrict__ act, const float *__restrict__ logp_old, const float *__restrict__ adv,
                                                    const float *__restrict__ ret, const int64_t *__restrict__ perm, int64_t start, int64_t count, int D, int n_h1,
                                                    int n_h2, const float *__restrict__ params, float clip, float *__restrict__ partial) {
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

// The gradient launch of pcc_ppo_minibatch_step_pop: blockIdx.y = member.  Member m runs the body above on its own permutation
// row, parameter block, clip (hyper[m][1]) and slice of the partial-gradient scratch, with the grid a stand-alone call with the
// same `count` has in x: the same tiles per wavefront, the same order of additions, the same bits.
template <int DP, int H1P, int H2P>
__global__ __launch_bounds__((Cls<DP, H1P, H2P>::kWaves) * 64, 1) void ppo_grad_tiled_pop_kernel(
    const float *__restrict__ obs, const float *__restrict__ act, const float *__restrict__ logp_old,
    const float *__restrict__ adv, const float *__restrict__ ret, const int64_t *__restrict__ perm, int64_t perm_stride, int64_t start,
    int64_t count, int D, int n_h1, int n_h2, const float *__restrict__ params, int64_t param_stride, const float *__restrict__ hyper,
    float *__restrict__ partial, int64_t partial_stride) {
    const int64_t m = blockIdx.y;
    const int64_t *perm_m = perm + m * perm_stride;
    const float *params_m = params + m * param_stride;
    float *partial_m = partial + m * partial_stride;
    float clip = hyper[m * 8 + 1];
    // (the member's pointers are made here, once, in scalar registers: left to the scheduler, (128; 64, 32) spills six vector registers)
    asm volatile("" : "+s"(perm_m), "+s"(params_m), "+s"(partial_m), "+s"(clip));
    ppo_grad_tiled_body<DP, H1P, H2P>(obs, act, logp_old, adv, ret, perm_m, start, count, D, n_h1, n_h2, params_m, clip, partial_m);
}

template <int DP, int H1P, int H2P>
__device__ __forceinline__ void policy_act_tiled_body(const float *__restrict__ obs, int64_t n, int D, int n_h1, int n_h2, const float *__restrict__ params,
                                                      const float *__restrict__ noise, float *__restrict__ mean_out, float *__restrict__ act_out, float *__restrict__ logp_out,
                                                      float *__restrict__ value_out) {
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

// pcc_policy_act_pop for the tiled shapes: blockIdx.z = member, its rows and parameter block through offset pointers, n = the
// member's rows (tiles start at the member's first row, as in a stand-alone launch over them).
template <int DP, int H1P, int H2P>
__global__ __launch_bounds__((Cls<DP, H1P, H2P>::kWaves) * 64, 1) void policy_act_tiled_pop_kernel(
    const float *__restrict__ obs, int64_t n_member, int D, int n_h1, int n_h2, const float *__restrict__ params, int64_t param_stride,
    const float *__restrict__ noise, float *__restrict__ mean_out, float *__restrict__ act_out, float *__restrict__ logp_out,
    float *__restrict__ value_out) {
    const int64_t m = blockIdx.z, off = m * n_member;
    policy_act_tiled_body<DP, H1P, H2P>(obs + off * D, n_member, D, n_h1, n_h2, params + m * param_stride, noise ? noise + off : nullptr,
                                        mean_out ? mean_out + off : nullptr, act_out ? act_out + off : nullptr,
                                        logp_out ? logp_out + off : nullptr, value_out ? value_out + off : nullptr);
}

// ---- host side
// the population launches: the single launch's arguments with n / count per member, plus the member strides
struct GradPopArgs : GradArgs {   // perm, params, partial: member 0's; clip unused (hyper[m][1])
    int64_t perm_stride, param_stride, partial_stride;
    const float *hyper;
    int n_members;
};
struct ActPopArgs : ActArgs {     // n = a member's rows; every row pointer is the whole batch's
    int64_t param_stride;
    int n_members;
};

template <int DP, int H1P, int H2P>
inline int launch_class(const GradPopArgs &a, hipStream_t st, int *blocks_out) {
    using C = Cls<DP, H1P, H2P>;
    const int64_t tiles = (a.count + kTile - 1) / kTile;
    int64_t blocks = (tiles + C::kWaves - 1) / C::kWaves;
    if (blocks > kMaxGradBlocks) blocks = kMaxGradBlocks;
    *blocks_out = (int)blocks;
    hipLaunchKernelGGL((ppo_grad_tiled_pop_kernel<DP, H1P, H2P>), dim3((unsigned)blocks, (unsigned)a.n_members), dim3(C::kWaves * kWave), 0, st,
                       a.obs, a.act, a.logp_old, a.adv, a.ret, a.perm, a.perm_stride, a.start, a.count, a.D, a.h1, a.h2, a.params,
                       a.param_stride, a.hyper, a.partial, a.partial_stride);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <int DP, int H1P, int H2P>
inline int launch_class(const ActPopArgs &a, hipStream_t st, int *) {
    using C = Cls<DP, H1P, H2P>;
    const int64_t tiles = (a.n + kTile - 1) / kTile;
    int64_t blocks = (tiles + C::kWaves - 1) / C::kWaves;
    if (blocks > 128) blocks = 128;
    hipLaunchKernelGGL((policy_act_tiled_pop_kernel<DP, H1P, H2P>), dim3((unsigned)blocks, 2, (unsigned)a.n_members), dim3(C::kWaves * kWave), 0,
                       st, a.obs, a.n, a.D, a.h1, a.h2, a.params, a.param_stride, a.noise, a.mean_out, a.act_out, a.logp_out, a.value_out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

int launch_grad_pop_d32(const GradPopArgs &a, hipStream_t st, int *blocks_out);
int launch_grad_pop_d64(const GradPopArgs &a, hipStream_t st, int *blocks_out);
int launch_grad_pop_d128(const GradPopArgs &a, hipStream_t st, int *blocks_out);
int launch_act_pop_d32(const ActPopArgs &a, hipStream_t st);
int launch_act_pop_d64(const ActPopArgs &a, hipStream_t st);
int launch_act_pop_d128(const ActPopArgs &a, hipStream_t st);

inline int launch_grad_pop(const GradPopArgs &a, hipStream_t st, int *blocks_out) {
    if (!in_domain(a.D, a.h1, a.h2)) return -2;
    return a.D <= 32 ? launch_grad_pop_d32(a, st, blocks_out) : a.D <= 64 ? launch_grad_pop_d64(a, st, blocks_out) : launch_grad_pop_d128(a, st, blocks_out);
}
inline int launch_act_pop(const ActPopArgs &a, hipStream_t st) {
    if (!in_domain(a.D, a.h1, a.h2)) return -2;
    return a.D <= 32 ? launch_act_pop_d32(a, st) : a.D <= 64 ? launch_act_pop_d64(a, st) : launch_act_pop_d128(a, st);
}

}  // namespace pcc_tiles
