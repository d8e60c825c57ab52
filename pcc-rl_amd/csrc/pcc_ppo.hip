// pcc_ppo.hip -- the update half of the on-device PPO caller: one optimiser step of
// PPO1's objective (clipped surrogate + 0.5 * value error - ent_coef * entropy; stable-baselines' defaults as
// src/gym/stable_solve.py:52 uses them) on one minibatch of the rollout, for the reference's policy shape
// (src/gym/stable_solve.py:39-45: pi and vf MLPs, obs -> 32 -> 16 -> 1, tanh, state-independent log-std), as TWO
// launches instead of the ~150 small framework launches of forward + autograd + Adam:
//
//   ppo_grad_mfma_kernel  every contraction of forward and backward on the matrix cores, fp32 (v_mfma_f32_32x32x2_f32 /
//                     v_mfma_f32_16x16x4_f32: exact fp32): a layer is a small GEMM per tile of 64 samples, the weights are
//                     B operands held in registers, the activations A operands read sample-major from LDS, tanh and
//                     its derivative elementwise in the MFMA's C layout; the weight gradients dW = dZ^T X are contractions
//                     over the samples whose accumulators stay in registers over all tiles of a wavefront.  Every
//                     workgroup writes ONE partial gradient.  (The first version of this kernel evaluated the networks
//                     lane = sample with plain FMAs and only the weight gradients on MFMAs: 392 us per million samples
//                     with the weights as scalar operands -- every output unit waits for its scalar loads -- 579 with
//                     the weights broadcast from LDS; this one 328.  profiles/r03_experiments.json.)
//   ppo_adam_kernel   sums the partial gradients in a fixed order (deterministic), adds the entropy
//                     term, applies Adam (torch.optim.Adam's arithmetic), writes the parameters in place.
//
// ppo_grad_mfma_kernel is built for --arch 32,16 at the observation lengths of PCC_MFMA_OBS_LENGTHS (pcc_policy_dev.h: the layout
// of the parameter block, tanh_fast and the Gaussian log-probability are that header's too); every other shape of the supported domain
// (pcc_ppo_supported: up to 128 observations, hidden layers up to 64 wide) takes ppo_grad_tiled_kernel (pcc_mlp_tiles.h), the
// tiled generalisation with run-time sizes, which writes partial gradients of the same layout for the same ppo_adam_kernel.
//
// Plus the GAE recursion as one launch (thread = env, T steps backwards).  fp32 like the framework path; checked against
// torch autograd in tests/test_ppo.py.
//
// Every kernel's grid has a member dimension: pcc_ppo_minibatch_step / pcc_gae are pcc_ppo_minibatch_step_pop / pcc_gae_pop with one
// member (include/pcc_policy.h), through the same launch functions (launch_step, launch_gae).  What a stand-alone call has on the
// host -- clip, lr, ent_coef, gamma, lam -- is a kernel argument, read where the population's device array `hyper` is NULL.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcc_mlp_tiles.h"
#include "pcc_policy.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 2;
constexpr int kMaxBlocks = 512;   // 2 wavefronts each: one per SIMD of the chip, which is what ~480 registers allow

using pcc::PolicyLayout;
using pcc::tanh_fast;
using pcc::wave_sum;

constexpr int kS33 = 33, kS17 = 17;               // row strides of the sample-major LDS buffers: conflict-free both ways
constexpr int kBufFloats = kWave * kS33;          // one [64][33] operand buffer

// ======================================================================================
// ppo_grad_mfma_kernel: a layer is a small GEMM per tile of 64 samples: the weights are the B
// operands and stay in registers for the whole kernel (forward: W1^T, W2^T; backward: W2), the activations are the A
// operands, read sample-major from LDS, the results land in the MFMA's C layout (lane = output unit, registers = samples),
// where tanh, its derivative and the bias gradients are elementwise / per-lane sums; each layer's output goes back to LDS
// sample-major for the next contraction.  Per network and tile 144 MFMAs (fp32: v_mfma_f32_32x32x2_f32 /
// v_mfma_f32_16x16x4_f32), ~7 k cycles of the matrix pipe.
//   layouts (cdna_hip_programming.md): 32x32x2: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31], C: col = l & 31,
//   row = (r & 3) + 8 (r >> 2) + 4 (l >> 5); 16x16x4: A[l & 15][k = l >> 4], B[k = l >> 4][l & 15], C: col = l & 15,
//   row = 4 (l >> 4) + r.
// ======================================================================================
constexpr int kMfmaWaveLds = 3 * kBufFloats + 4 * kWave;   // x | h1 | dz (dz2, then dz1) | act, logp_old, adv, ret

__device__ __forceinline__ float row16_sum(float x) {   // the sum over the 16 lanes of a DPP row, in every lane of it
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xF, 0xF, false));    // quad_perm:[1,0,3,2]
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xF, 0xF, false));    // quad_perm:[2,3,0,1]
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xF, 0xF, false));   // row_half_mirror
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x140, 0xF, 0xF, false));   // row_mirror
    return x;
}

struct MfmaWeights {   // one network's weights as MFMA B operands (and per-lane constants of the C layout)
    float w1b[16];     // layer 1 forward:  W1[n = l & 31][k = 2 t + (l >> 5)]
    float w2b[8];      // layer 2 forward:  W2[n = l & 15][k = 4 t + (l >> 4)]
    float w2c[8];      // layer 2 backward: W2[j = 2 t + (l >> 5)][n = l & 31]
    float b1c, b2c, w3c, b3;
};
struct MfmaAcc {       // one network's gradient sums of a wavefront
    f32x16 w1;         // dW1: row = unit (C layout of 32x32), col = feature
    f32x4 w2a, w2b;    // dW2: row = unit j (C layout of 16x16), col = k (+ 16)
    float b1, b2, w3, b3;   // per-lane partial sums: b1 for unit l & 31, b2 / w3 for unit l & 15, b3 (lanes with l & 15 == 0 count)
};

template <int D, int H1, int H2>
__device__ __forceinline__ void mfma_load_weights(MfmaWeights &w, const float *__restrict__ p, uint32_t lane) {
    constexpr PolicyLayout L(D, H1, H2);
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const uint32_t k = 2u * t + (lane >> 5);
        w.w1b[t] = k < (uint32_t)D ? p[L.W1 + (lane & 31u) * D + k] : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < 8; t++) {
        w.w2b[t] = p[L.W2 + (lane & 15u) * H1 + 4u * t + (lane >> 4)];
        w.w2c[t] = p[L.W2 + (2u * t + (lane >> 5)) * H1 + (lane & 31u)];
    }
    w.b1c = p[L.B1 + (lane & 31u)];
    w.b2c = p[L.B2 + (lane & 15u)];
    w.w3c = p[L.W3 + (lane & 15u)];
    w.b3 = p[L.B3];
}

// forward of one network over the tile: on return h1 (C layout of two 32x32 tiles) and h2 (C layout of four 16x16 tiles) hold
// the activations, H1s holds h1 sample-major, out[T4][r] the network's output for sample 16 T4 + 4 (l >> 4) + r
template <int D, int H1, int H2>
__device__ __forceinline__ void mfma_forward(const MfmaWeights &w, const float *Xs, float *H1s, uint32_t lane, float (&h1)[2][16],
                                             float (&h2)[4][4], float (&out)[4][4]) {
#pragma unroll
    for (int T = 0; T < 2; T++) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = w.b1c;
#pragma unroll
        for (int t = 0; t < 16; t++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Xs[(32u * T + (lane & 31u)) * kS33 + 2u * t + (lane >> 5)], w.w1b[t], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            h1[T][r] = tanh_fast(acc[r]);
            const uint32_t m = 32u * T + (uint32_t)(r & 3) + 8u * (uint32_t)(r >> 2) + 4u * (lane >> 5);
            H1s[m * kS33 + (lane & 31u)] = h1[T][r];
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int T4 = 0; T4 < 4; T4++) {
        f32x4 acc;
#pragma unroll
        for (int r = 0; r < 4; r++) acc[r] = w.b2c;
#pragma unroll
        for (int t = 0; t < 8; t++)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(H1s[(16u * T4 + (lane & 15u)) * kS33 + 4u * t + (lane >> 4)], w.w2b[t], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            h2[T4][r] = tanh_fast(acc[r]);
            out[T4][r] = row16_sum(h2[T4][r] * w.w3c) + w.b3;   // the 16 lanes of a DPP row = the 16 units of one sample
        }
    }
}

// backward of one network over the tile, given d loss / d output per sample (dout[T4][r], like `out` above)
template <int D, int H1, int H2>
__device__ __forceinline__ void mfma_backward(const MfmaWeights &w, MfmaAcc &g, const float *Xs, const float *H1s, float *Zs,
                                              uint32_t lane, const float (&h1)[2][16], const float (&h2)[4][4],
                                              const float (&dout)[4][4]) {
    // ---- layer 3 and the pre-activation gradient of layer 2 (C layout of the 16x16 tiles), sample-major to LDS
#pragma unroll
    for (int T4 = 0; T4 < 4; T4++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float d = dout[T4][r];
            const float dz2 = d * w.w3c * (1.0f - h2[T4][r] * h2[T4][r]);
            g.w3 = fmaf(d, h2[T4][r], g.w3);
            g.b2 += dz2;
            if ((lane & 15u) == 0u) g.b3 += d;
            const uint32_t m = 16u * T4 + 4u * (lane >> 4) + (uint32_t)r;
            Zs[m * kS17 + (lane & 15u)] = dz2;
        }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- dW2[j][k] += sum_s dz2[s][j] h1[s][k]
#pragma unroll 4
    for (int t = 0; t < kWave / 4; t++) {
        const uint32_t s = 4u * t + (lane >> 4);
        const float a = Zs[s * kS17 + (lane & 15u)];
        g.w2a = __builtin_amdgcn_mfma_f32_16x16x4f32(a, H1s[s * kS33 + (lane & 15u)], g.w2a, 0, 0, 0);
        g.w2b = __builtin_amdgcn_mfma_f32_16x16x4f32(a, H1s[s * kS33 + 16u + (lane & 15u)], g.w2b, 0, 0, 0);
    }
    // ---- dh1[s][k] = sum_j dz2[s][j] W2[j][k]; dz1 = dh1 (1 - h1^2) (C layout of the 32x32 tiles)
    float dz1[2][16];
#pragma unroll
    for (int T = 0; T < 2; T++) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
        for (int t = 0; t < 8; t++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Zs[(32u * T + (lane & 31u)) * kS17 + 2u * t + (lane >> 5)], w.w2c[t], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            dz1[T][r] = acc[r] * (1.0f - h1[T][r] * h1[T][r]);
            g.b1 += dz1[T][r];
        }
    }
    __builtin_amdgcn_wave_barrier();   // (every read of dz2 is issued: dz1 takes the buffer over)
#pragma unroll
    for (int T = 0; T < 2; T++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const uint32_t m = 32u * T + (uint32_t)(r & 3) + 8u * (uint32_t)(r >> 2) + 4u * (lane >> 5);
            Zs[m * kS33 + (lane & 31u)] = dz1[T][r];
        }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- dW1[i][k] += sum_s dz1[s][i] x[s][k]
#pragma unroll 8
    for (int t = 0; t < kWave / 2; t++) {
        const uint32_t s = 2u * t + (lane >> 5);
        g.w1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Zs[s * kS33 + (lane & 31u)], Xs[s * kS33 + (lane & 31u)], g.w1, 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
}

template <int D, int H1, int H2>
__device__ __forceinline__ void mfma_acc_store(const MfmaAcc &acc, float *g, const uint32_t lane, const bool add) {
    constexpr PolicyLayout L(D, H1, H2);
    auto put = [&](int idx, float v) { g[idx] = add ? g[idx] + v : v; };
    const uint32_t col = lane & 31u;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const uint32_t row = (uint32_t)(r & 3) + 8u * (uint32_t)(r >> 2) + 4u * (lane >> 5);
        if (col < (uint32_t)D) put(L.W1 + (int)row * D + (int)col, acc.w1[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t row = 4u * (lane >> 4) + (uint32_t)r, c = lane & 15u;
        put(L.W2 + (int)row * H1 + (int)c, acc.w2a[r]);
        put(L.W2 + (int)row * H1 + 16 + (int)c, acc.w2b[r]);
    }
    float b1 = acc.b1, b2 = acc.b2, w3 = acc.w3;
    b1 += __shfl_xor(b1, 32, kWave);
    b2 += __shfl_xor(b2, 16, kWave); b2 += __shfl_xor(b2, 32, kWave);
    w3 += __shfl_xor(w3, 16, kWave); w3 += __shfl_xor(w3, 32, kWave);
    const float b3 = wave_sum(acc.b3);
    if (lane < 32u) put(L.B1 + (int)lane, b1);
    if (lane < 16u) { put(L.B2 + (int)lane, b2); put(L.W3 + (int)lane, w3); }
    if (lane == 0u) put(L.B3, b3);
}

// blockIdx.y = member of a population (a stand-alone call is a population of one: pcc_ppo_minibatch_step launches gridDim.y = 1 with
// hyper == NULL and its clip as an argument).  Member m works on its own permutation row (perm_all may be NULL: the samples in
// order), parameter block, clip (hyper[m][1]) and slice of the partial-gradient scratch; gridDim.x depends on `count` alone, so
// every wavefront walks the same tiles and every sum has the same order whatever the number of members: the same bits.
template <int D, int H1, int H2>
__global__ __launch_bounds__(kWavesPerBlock *kWave, 1) void ppo_grad_mfma_kernel(
    const float *__restrict__ obs, const float *__restrict__ act, const float *__restrict__ logp_old,
    const float *__restrict__ adv, const float *__restrict__ ret, const int64_t *__restrict__ perm_all, int64_t perm_stride,
    int64_t start, int64_t count, const float *__restrict__ params_all, int64_t param_stride, const float *__restrict__ hyper,
    float clip_arg, float *__restrict__ partial_all, int64_t partial_stride) {
    const int64_t member = blockIdx.y;
    const int64_t *__restrict__ perm = perm_all ? perm_all + member * perm_stride : nullptr;
    const float *__restrict__ params = params_all + member * param_stride;
    float *__restrict__ partial = partial_all + member * partial_stride;
    const float clip = hyper ? hyper[member * 8 + 1] : clip_arg;
    constexpr PolicyLayout L(D, H1, H2);
    static_assert(H1 == 32 && H2 == 16 && D <= 32, "the MFMA tiles are the reference's --arch 32,16 on at most 32 features");
    constexpr int kPi = 0, kLogStd = L.log_std(), kVf = L.vf(), kParams = L.n_params();
    static_assert(kParams + 4 <= kMfmaWaveLds, "the block's gradient is reduced in a wavefront's LDS buffers");
    __shared__ float lds[kWavesPerBlock * kMfmaWaveLds];
    const uint32_t lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    float *Xs = lds + wv * kMfmaWaveLds, *H1s = Xs + kBufFloats, *Zs = H1s + kBufFloats, *Sc = Zs + kBufFloats;
    const float log_std = params[kLogStd];
    const float inv_std = __expf(-log_std);
    const float inv_n = 1.0f / (float)count;
    // both networks' weights stay in registers (~480 with the activations of a tile: one wavefront per SIMD.  One network
    // at a time -- two passes over the samples, two wavefronts per SIMD at 256 registers -- was measured: 506 us against
    // 328 per million samples, spills and a second gather of the observation rows)
    MfmaWeights wpi, wvf;
    mfma_load_weights<D, H1, H2>(wpi, params + kPi, lane);
    mfma_load_weights<D, H1, H2>(wvf, params + kVf, lane);
    MfmaAcc gpi, gvf;
#pragma unroll
    for (int r = 0; r < 16; r++) { gpi.w1[r] = 0.0f; gvf.w1[r] = 0.0f; }
#pragma unroll
    for (int r = 0; r < 4; r++) { gpi.w2a[r] = gpi.w2b[r] = 0.0f; gvf.w2a[r] = gvf.w2b[r] = 0.0f; }
    gpi.b1 = gpi.b2 = gpi.w3 = gpi.b3 = 0.0f;
    gvf.b1 = gvf.b2 = gvf.w3 = gvf.b3 = 0.0f;
    float g_logstd = 0.0f, s_pg = 0.0f, s_vf = 0.0f, s_clip = 0.0f;
    const int64_t n_tiles = (count + kWave - 1) / kWave;
    for (int64_t tile = (int64_t)blockIdx.x * kWavesPerBlock + wv; tile < n_tiles; tile += (int64_t)gridDim.x * kWavesPerBlock) {
        // ---- the tile's samples, sample-major in LDS (lane = sample for the loads only)
        {
            const int64_t k = tile * kWave + lane;
            const bool valid = k < count;
            const int64_t idx = valid ? (perm ? perm[start + k] : start + k) : 0;
            if constexpr (D % 2 == 0) {
                const float2 *row = reinterpret_cast<const float2 *>(obs + idx * D);   // D even: 8-byte aligned rows
#pragma unroll
                for (int j = 0; j < D / 2; j++) {
                    const float2 v = row[j];
                    Xs[lane * kS33 + 2 * j] = valid ? v.x : 0.0f;
                    Xs[lane * kS33 + 2 * j + 1] = valid ? v.y : 0.0f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < D; j++) Xs[lane * kS33 + j] = valid ? obs[idx * D + j] : 0.0f;
            }
#pragma unroll
            for (int j = D; j < 32; j++) Xs[lane * kS33 + j] = 0.0f;
            Sc[lane] = valid ? act[idx] : 0.0f;
            Sc[kWave + lane] = valid ? logp_old[idx] : 0.0f;
            Sc[2 * kWave + lane] = valid ? adv[idx] : 0.0f;
            Sc[3 * kWave + lane] = valid ? ret[idx] : 0.0f;
        }
        __builtin_amdgcn_wave_barrier();
        const int64_t left = count - tile * kWave;   // samples of this tile that exist
        float h1[2][16], h2[4][4], out[4][4], dout[4][4];
        // ---- policy network: log-probability of the taken action, clipped surrogate.  The per-sample arithmetic below is
        // written out in ppo_grad_tiled_kernel (pcc_mlp_tiles.h) too and the two are kept in step by hand: as one shared
        // function (sums by reference) the results are the same but two tiled instantiations change their register counts.
        mfma_forward<D, H1, H2>(wpi, Xs, H1s, lane, h1, h2, out);
#pragma unroll
        for (int T4 = 0; T4 < 4; T4++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t m = 16u * T4 + 4u * (lane >> 4) + (uint32_t)r;
                const bool valid = (int64_t)m < left;
                const float a = Sc[m], lp_old = Sc[kWave + m], ad = Sc[2 * kWave + m];
                const float z = (a - out[T4][r]) * inv_std;
                const float lp = pcc::gaussian_logp(z, log_std);
                const float ratio = __expf(lp - lp_old);
                const float lo = 1.0f - clip, hi = 1.0f + clip;
                const float rc = fminf(fmaxf(ratio, lo), hi);
                const float surr1 = ratio * ad, surr2 = rc * ad;
                const bool through = surr1 <= surr2;   // min picks the unclipped term (inside the range both are the same)
                const float dlp = (valid && through) ? -ad * ratio * inv_n : 0.0f;
                dout[T4][r] = dlp * z * inv_std;
                if (valid && (lane & 15u) == 0u) {   // (the 16 lanes of a row hold the same sample: one of them counts)
                    g_logstd += dlp * (z * z - 1.0f);
                    s_pg += fminf(surr1, surr2);
                    s_clip += (ratio < lo || ratio > hi) ? 1.0f : 0.0f;
                }
            }
        }
        mfma_backward<D, H1, H2>(wpi, gpi, Xs, H1s, Zs, lane, h1, h2, dout);
        // ---- value network: 0.5 * mean((v - ret)^2)
        mfma_forward<D, H1, H2>(wvf, Xs, H1s, lane, h1, h2, out);
#pragma unroll
        for (int T4 = 0; T4 < 4; T4++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t m = 16u * T4 + 4u * (lane >> 4) + (uint32_t)r;
                const bool valid = (int64_t)m < left;
                const float err = valid ? out[T4][r] - Sc[3 * kWave + m] : 0.0f;
                dout[T4][r] = err * inv_n;
                if ((lane & 15u) == 0u) s_vf += err * err;
            }
        }
        mfma_backward<D, H1, H2>(wvf, gvf, Xs, H1s, Zs, lane, h1, h2, dout);
    }
    // ---- the block's partial gradient: every wavefront's sums -> LDS (wavefront 0's buffers), one after the other
    __syncthreads();
    float *g = lds;
    for (uint32_t w = 0; w < (uint32_t)kWavesPerBlock; w++) {
        if (wv == w) {
            mfma_acc_store<D, H1, H2>(gpi, g + kPi, lane, w != 0);
            mfma_acc_store<D, H1, H2>(gvf, g + kVf, lane, w != 0);
            const float gl = wave_sum(g_logstd), a = wave_sum(s_pg), b = wave_sum(s_vf), c = wave_sum(s_clip);
            if (lane == 0) {
                g[kLogStd] = (w ? g[kLogStd] : 0.0f) + gl;
                g[kParams + 0] = (w ? g[kParams + 0] : 0.0f) + a;
                g[kParams + 1] = (w ? g[kParams + 1] : 0.0f) + b;
                g[kParams + 2] = (w ? g[kParams + 2] : 0.0f) + c;
                g[kParams + 3] = 0.0f;
            }
        }
        __syncthreads();
    }
    float *out_p = partial + (int64_t)blockIdx.x * (kParams + 4);
    for (int k = threadIdx.x; k < kParams + 4; k += blockDim.x) out_p[k] = g[k];
}

// 16 parameters per workgroup: thread (r, c) sums parameter c's partial gradients of the blocks r, r + 16, ..., the 16 row sums
// are added in order (deterministic: no atomics anywhere); then the entropy term (entropy of the diagonal Gaussian = const +
// log_std: d/d log_std of -ent_coef * entropy is -ent_coef) and Adam as torch.optim.Adam computes it.  blockIdx.y = member, with
// its lr and entropy coefficient from hyper[m] (hyper == NULL: the stand-alone call's arguments); the bias corrections are the
// host's (one adam_step for all members; a member with lr == 0 returns before it reads them, and its moments may be NULL).
__global__ __launch_bounds__(256) void ppo_adam_kernel(const float *__restrict__ partial_all, int64_t partial_stride, int n_blocks,
                                                       int n_params, int logstd_index, const float *__restrict__ hyper,
                                                       float ent_coef_arg, float lr_arg, float *__restrict__ params_all,
                                                       float *__restrict__ m_all, float *__restrict__ v_all, int64_t param_stride,
                                                       float beta1, float beta2, float eps, float bias1, float bias2_sqrt,
                                                       float inv_count, float *__restrict__ grad_all, float *__restrict__ stats_all) {
    const int64_t mb = blockIdx.y, po = mb * param_stride;
    const float *__restrict__ partial = partial_all + mb * partial_stride;
    float *__restrict__ params = params_all + po;
    float *__restrict__ m = m_all ? m_all + po : nullptr, *__restrict__ v = v_all ? v_all + po : nullptr;
    float *__restrict__ grad_out = grad_all ? grad_all + po : nullptr, *__restrict__ stats_out = stats_all ? stats_all + mb * 4 : nullptr;
    const float lr = hyper ? hyper[mb * 8 + 0] : lr_arg, ent_coef = hyper ? hyper[mb * 8 + 2] : ent_coef_arg;
    __shared__ float rows[16][17];
    const int c = threadIdx.x & 15, r = threadIdx.x >> 4;
    const int p = blockIdx.x * 16 + c;
    const int stride = n_params + 4;
    float g = 0.0f;
    if (p < stride)
        for (int b = r; b < n_blocks; b += 16) g += partial[(int64_t)b * stride + p];
    rows[r][c] = g;
    __syncthreads();
    if (r != 0 || p >= stride) return;
    g = rows[0][c];
#pragma unroll
    for (int k = 1; k < 16; k++) g += rows[k][c];
    if (p >= n_params) {   // {-policy loss, 2 * value loss, clipped fraction, -} as means over the minibatch
        if (stats_out) stats_out[p - n_params] = g * inv_count;
        return;
    }
    if (p == logstd_index) g -= ent_coef;
    if (grad_out) grad_out[p] = g;
    if (lr == 0.0f) return;   // gradient only
    const float mm = beta1 * m[p] + (1.0f - beta1) * g;
    const float vv = beta2 * v[p] + (1.0f - beta2) * g * g;
    m[p] = mm;
    v[p] = vv;
    const float denom = sqrtf(vv) / bias2_sqrt + eps;
    params[p] -= (lr / bias1) * (mm / denom);
}

// Generalised advantage estimation over [T][N] rollout rows (thread = env, backwards in time): dones[t] marks that the
// env was reset after step t.  blockIdx.y = member, which owns n_member consecutive columns of the [T][n] rows and reads its
// own gamma and lambda (hyper[m][3], [4]; hyper == NULL: the stand-alone call's arguments, one member of all n columns).
__global__ void gae_kernel(const float *__restrict__ rew, const float *__restrict__ val, const uint8_t *__restrict__ done,
                           const float *__restrict__ last_val, int T, int64_t n, int64_t n_member, const float *__restrict__ hyper,
                           float gamma_arg, float lam_arg, float *__restrict__ adv, float *__restrict__ ret) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_member) return;
    const int64_t i = (int64_t)blockIdx.y * n_member + r;
    const float gamma = hyper ? hyper[blockIdx.y * 8 + 3] : gamma_arg, lam = hyper ? hyper[blockIdx.y * 8 + 4] : lam_arg;
    float next_v = last_val[i], run = 0.0f;
    for (int t = T - 1; t >= 0; t--) {
        const int64_t k = (int64_t)t * n + i;
        const float alive = done[k] ? 0.0f : 1.0f;
        const float v = val[k];
        const float delta = rew[k] + gamma * next_v * alive - v;
        run = delta + gamma * lam * alive * run;
        adv[k] = run;
        ret[k] = run + v;
        next_v = v;
    }
}

}  // namespace

// the shapes ppo_grad_mfma_kernel is instantiated for; the rest of the domain goes to the tiled kernel
static bool mfma_fixed_shape(int obs_dim, int h1, int h2) { return h1 == 32 && h2 == 16 && pcc::mfma_grad_length(obs_dim); }

extern "C" int pcc_ppo_supported(int obs_dim, int h1, int h2) { return pcc_tiles::in_domain(obs_dim, h1, h2) ? 1 : 0; }

extern "C" int pcc_ppo_scratch_floats(int obs_dim, int h1, int h2) {
    const int blocks = mfma_fixed_shape(obs_dim, h1, h2) || !pcc_tiles::in_domain(obs_dim, h1, h2) ? kMaxBlocks : pcc_tiles::kMaxGradBlocks;
    return blocks * (PolicyLayout(obs_dim, h1, h2).n_params() + 4);
}

// One optimiser step of a.n_members learners (both entry points; the arguments are checked there): the gradient launch, then the
// Adam launch.  a.hyper != NULL: lr, clip and ent_coef are the members' rows of it and every member may update; NULL: the arguments.
static int launch_step(pcc_tiles::GradArgs a, float *params, float *adam_m, float *adam_v, int adam_step, float lr, float beta1,
                       float beta2, float eps, float ent_coef, float *grad_out, float *stats_out, hipStream_t st) {
    if (!pcc_tiles::in_domain(a.D, a.h1, a.h2)) return -2;   // (the caller falls back to its framework path)
    const PolicyLayout L(a.D, a.h1, a.h2);
    a.partial_stride = pcc_ppo_scratch_floats(a.D, a.h1, a.h2);
    int blocks = 0;
    if (mfma_fixed_shape(a.D, a.h1, a.h2)) {
        const int64_t tiles = (a.count + kWave - 1) / kWave;
        const int64_t nb = (tiles + kWavesPerBlock - 1) / kWavesPerBlock;
        blocks = nb > kMaxBlocks ? kMaxBlocks : (int)nb;
        const dim3 grid((unsigned)blocks, (unsigned)a.n_members), block(kWavesPerBlock * kWave);
#define PCC_PPO_CASE(DD)                                                                                                        \
    if (a.D == DD)                                                                                                              \
        hipLaunchKernelGGL((ppo_grad_mfma_kernel<DD, 32, 16>), grid, block, 0, st, a.obs, a.act, a.logp_old, a.adv, a.ret, a.perm, \
                           a.perm_stride, a.start, a.count, a.params, a.param_stride, a.hyper, a.clip, a.partial, a.partial_stride);
        PCC_MFMA_OBS_LENGTHS(PCC_PPO_CASE)
#undef PCC_PPO_CASE
    } else {   // any other shape of the domain: the tiled kernel
        const int rc = pcc_tiles::launch_grad(a, st, &blocks);
        if (rc != 0) return rc;
    }
    if (hipGetLastError() != hipSuccess) return -3;
    const bool update = a.hyper || lr != 0.0f;
    const float bias1 = update ? 1.0f - powf(beta1, (float)adam_step) : 1.0f;
    const float bias2 = update ? sqrtf(1.0f - powf(beta2, (float)adam_step)) : 1.0f;
    hipLaunchKernelGGL(ppo_adam_kernel, dim3((unsigned)((L.n_params() + 4 + 15) / 16), (unsigned)a.n_members), dim3(256), 0, st, a.partial,
                       a.partial_stride, blocks, L.n_params(), L.log_std(), a.hyper, ent_coef, lr, params, adam_m, adam_v, a.param_stride,
                       beta1, beta2, eps, bias1, bias2, 1.0f / (float)a.count, grad_out, stats_out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

static int launch_gae(const float *rewards, const float *values, const uint8_t *dones, const float *last_value, int T, int64_t n_envs,
                      int n_members, const float *hyper, float gamma, float lam, float *adv_out, float *ret_out, void *stream) {
    const int64_t n_member = n_envs / n_members;
    hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((n_member + 255) / 256), (unsigned)n_members), dim3(256), 0,
                       static_cast<hipStream_t>(stream), rewards, values, dones, last_value, T, n_envs, n_member, hyper, gamma, lam,
                       adv_out, ret_out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int pcc_ppo_minibatch_step(const float *obs, const float *act, const float *logp_old, const float *adv,
                                      const float *ret, const int64_t *perm, int64_t start, int64_t count, int obs_dim,
                                      int h1, int h2, float *params, float *adam_m, float *adam_v, int adam_step, float lr,
                                      float beta1, float beta2, float eps, float clip, float ent_coef, float *scratch,
                                      float *grad_out, float *stats_out, void *stream) {
    if (!obs || !act || !logp_old || !adv || !ret || !params || !scratch || count < 1 || start < 0) return -1;
    if (lr != 0.0f && (!adam_m || !adam_v || adam_step < 1)) return -1;
    const pcc_tiles::GradArgs a{obs, act, logp_old, adv, ret, perm, 0, start, count, obs_dim, h1, h2, params, 0, nullptr, clip, scratch, 0, 1};
    return launch_step(a, params, adam_m, adam_v, adam_step, lr, beta1, beta2, eps, ent_coef, grad_out, stats_out,
                       static_cast<hipStream_t>(stream));
}

extern "C" int pcc_gae(const float *rewards, const float *values, const uint8_t *dones, const float *last_value, int T,
                       int64_t n_envs, float gamma, float lam, float *adv_out, float *ret_out, void *stream) {
    if (!rewards || !values || !dones || !last_value || !adv_out || !ret_out || T < 1 || n_envs < 1) return -1;
    return launch_gae(rewards, values, dones, last_value, T, n_envs, 1, nullptr, gamma, lam, adv_out, ret_out, stream);
}

extern "C" int pcc_ppo_minibatch_step_pop(const float *obs, const float *act, const float *logp_old, const float *adv,
                                          const float *ret, const int64_t *perm, int64_t perm_stride, int64_t start, int64_t count,
                                          int obs_dim, int h1, int h2, float *params, float *adam_m, float *adam_v,
                                          int64_t param_stride, int n_members, const float *hyper, int adam_step, float beta1,
                                          float beta2, float eps, float *scratch, float *grad_out, float *stats_out, void *stream) {
    if (!obs || !act || !logp_old || !adv || !ret || !perm || !params || !scratch || !hyper || count < 1 || start < 0) return -1;
    if (!adam_m || !adam_v || adam_step < 1) return -1;   // (the learning rates are on the device: every member may update)
    if (n_members < 1 || n_members > 1024 || perm_stride < 0) return -1;
    if (!pcc_tiles::in_domain(obs_dim, h1, h2)) return -2;
    if (param_stride < PolicyLayout(obs_dim, h1, h2).n_params() || param_stride % 64 != 0) return -1;
    const pcc_tiles::GradArgs a{obs, act, logp_old, adv, ret, perm, perm_stride, start, count, obs_dim, h1, h2, params, param_stride,
                                hyper, 0.0f, scratch, 0, n_members};
    return launch_step(a, params, adam_m, adam_v, adam_step, 0.0f, beta1, beta2, eps, 0.0f, grad_out, stats_out,
                       static_cast<hipStream_t>(stream));
}

extern "C" int pcc_gae_pop(const float *rewards, const float *values, const uint8_t *dones, const float *last_value, int T,
                           int64_t n_envs, int n_members, const float *hyper, float *adv_out, float *ret_out, void *stream) {
    if (!rewards || !values || !dones || !last_value || !hyper || !adv_out || !ret_out || T < 1 || n_envs < 1) return -1;
    if (n_members < 1 || n_members > 1024 || n_envs % n_members != 0) return -1;
    return launch_gae(rewards, values, dones, last_value, T, n_envs, n_members, hyper, 0.0f, 0.0f, adv_out, ret_out, stream);
}
