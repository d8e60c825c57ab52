// pcc_policy_dev.h -- what every kernel of the policy (the reference's pi / vf MLPs with a Gaussian head) shares, once: the layout
// of the parameter block (PolicyLayout), the table of observation lengths with a fully unrolled kernel, tanh_fast, wave_sum, the
// Gaussian head, and the policy forward inside the env's kernels (policy_group: the rollout epilogue of pcc_retire.hip and
// pcc_small.hip, pcc_rollout).  The stand-alone forward (pcc_policy.hip), the gradient kernels (pcc_ppo.hip, pcc_mlp_tiles.h)
// and the epilogue must agree bit for bit (include/pcc_sim.h: pcc_rollout), which is why none of them has a copy of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcc {

// The parameter block (include/pcc_policy.h), floats: pi {W1[h1][D], b1[h1], W2[h2][h1], b2[h2], W3[h2], b3, log_std}, then vf
// {the same without log_std}.  W1 .. B3 are offsets inside one network's N floats; the pi network starts at 0, vf at vf().
struct PolicyLayout {
    int D, h1, h2;
    int W1, B1, W2, B2, W3, B3, N;
    __host__ __device__ constexpr PolicyLayout(int D_, int h1_, int h2_)
        : D(D_), h1(h1_), h2(h2_), W1(0), B1(h1_ * D_), W2(B1 + h1_), B2(W2 + h2_ * h1_), W3(B2 + h2_), B3(W3 + h2_), N(B3 + 1) {}
    // (functions, not fields: with run-time sizes they are then computed where they are used, as the kernels always did -- as
    // fields, computed at construction, they moved instructions in the tiled gradient kernels)
    __host__ __device__ constexpr int log_std() const { return N; }
    __host__ __device__ constexpr int vf() const { return N + 1; }
    __host__ __device__ constexpr int n_params() const { return 2 * N + 1; }
};
static_assert(PolicyLayout(30, 32, 16).N == 1537 && PolicyLayout(30, 32, 16).n_params() == 3075, "the reference's policy");
static_assert(PolicyLayout(30, 32, 16).B1 == 960 && PolicyLayout(30, 32, 16).W2 == 992 && PolicyLayout(30, 32, 16).B2 == 1504 &&
              PolicyLayout(30, 32, 16).W3 == 1520 && PolicyLayout(30, 32, 16).B3 == 1536, "W1, b1, W2, b2, W3, b3 in this order");
static_assert(PolicyLayout(7, 5, 3).vf() == PolicyLayout(7, 5, 3).log_std() + 1 && PolicyLayout(1, 1, 1).n_params() == 13, "pi, log_std, vf");

// The observation lengths with a fully unrolled kernel for the reference's --arch 32,16: policy_act_fixed_kernel<D, 32, 16> (and
// the generic policy_act_kernel<D> for other small policies) at all of them, ppo_grad_mfma_kernel<D, 32, 16> at those of at most
// 32 observations -- each ONE kernel for the stand-alone and the population entry points (the member is a grid dimension).  Every dispatch is generated from these lists; pcc_rollout runs --arch 32,16 at these lengths only.
#define PCC_MFMA_OBS_LENGTHS(X) X(30) X(3) X(6) X(12)   // 30 = history 10 x 3 features: the reference's default observation (ns:382-388)
#define PCC_FIXED_OBS_LENGTHS(X) PCC_MFMA_OBS_LENGTHS(X) X(36) X(60)   // 36 = history 3 x all 12 features
#define PCC_FIXED_OBS_LENGTHS_TEXT "3, 6, 12, 30, 36 or 60"             // (the same lengths, for messages)
#define PCC_OBS_LENGTH_IS(DD) || D == DD
constexpr bool fixed_act_length(int D) { return false PCC_FIXED_OBS_LENGTHS(PCC_OBS_LENGTH_IS); }
constexpr bool mfma_grad_length(int D) { return false PCC_MFMA_OBS_LENGTHS(PCC_OBS_LENGTH_IS); }
#undef PCC_OBS_LENGTH_IS
static_assert(fixed_act_length(36) && !mfma_grad_length(36) && mfma_grad_length(30) && !fixed_act_length(21), "the two lists");

// tanh(x) = 1 - 2 / (exp(2x) + 1) by the hardware's exp2 and reciprocal: absolute error ~1e-7 (one rounding of the quotient
// against 1), saturates cleanly; a fifth of libm's tanhf in instructions (48 of them per network and env: half of the fixed
// kernel's time went into them).  The rollout's and the update's forward are this one function.
__device__ __forceinline__ float tanh_fast(float x) {
    const float e = __expf(2.0f * x);
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The state-independent log-std Gaussian head, two functions because every caller tests its output pointers for NULL in between:
// the action sampled with the standard-normal draw eps (0: the mean itself), and log N(a; mu, sigma) = -z^2 / 2 - log_std -
// log(2 pi) / 2 at z = (a - mu) / sigma -- which is eps for the sampled action (the forward kernels) and computed from the stored
// action in the gradient kernels.  expf (libm's), not __expf.
constexpr float kHalfLog2Pi = 0.918938533204672742f;
__device__ __forceinline__ float gaussian_act(float mu, float log_std, float eps) { return mu + expf(log_std) * eps; }
__device__ __forceinline__ float gaussian_logp(float z, float log_std) { return -0.5f * z * z - log_std - kHalfLog2Pi; }

// The epilogue's network: the reference's --arch 32,16 (pcc_policy_act's fixed kernel), any observation length up to 64.
constexpr int kPolH1 = 32, kPolH2 = 16;
constexpr int kPolScratch = 64;   // LDS floats per env of the epilogue: the observation row, then layer 1's, then layer 2's outputs

// What a launch with the policy in its epilogue computes (pcc_rollout): after its step s (0-based within the launch) the env's
// next action -- the policy on the observation row the step just wrote -- goes to row t0 + s + 1 of act / logp / value, with
// noise row t0 + s + 1 (noise NULL: deterministic).  Rows are [N] (one sender).  act has act_rows rows used round robin
// (0 = a row per step); the small-batch kernel's send part reads its actions from there too (row t0 + s).
struct PolicyArgs {
    const float *params;   // pcc_policy_act's parameter block (include/pcc_policy.h), device
    int n_params;
    int D;                 // observation length (<= kPolScratch: the row is staged there)
    int act_rows;
    int t0;
    const float *noise;
    float *act, *logp, *value;
};

__device__ __forceinline__ int64_t pol_act_row(const PolicyArgs &P, int t) { return P.act_rows ? t % P.act_rows : t; }

// LDS is written by some lanes of a group and read by others of the same wavefront
__device__ __forceinline__ void pol_group_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The policy for env i of n by the G lanes of its group (gl = lane in the group), G = 8 or 16, into row t of the outputs: w = the
// parameter block staged in LDS, xs = the env's kPolScratch floats of LDS, obs_row = the observation row this group's lanes have
// just stored.  Every hidden unit is one lane's ordered chain of fmaf from its bias, k = 0 .. D-1 (units, not k, are spread over
// the lanes), then tanh_fast; the output is b3 plus an ordered fmaf over the 16 z2: the operations of
// policy_act_fixed_kernel<D, 32, 16>, in its order, so the same bits (the build has -ffp-contract=off).
template <int G>
__device__ __forceinline__ void policy_group(const PolicyArgs &P, const float *w, float *xs, const float *obs_row, int64_t i,
                                             int64_t n, uint32_t gl, int t) {
    static_assert(G == 8 || G == 16, "8 or 16 lanes per env");
    constexpr int U1 = 2 * kPolH1 / G, U2 = 2 * kPolH2 / G;
    const int D = P.D;
    const PolicyLayout L(D, kPolH1, kPolH2);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the row's stores (other lanes of this group) before its loads
    for (int x = (int)gl; x < D; x += G) xs[x] = obs_row[x];
    pol_group_sync();
    // layer 1: unit j = gl + u G of the 64 (pi 0..31, vf 32..63)
    float acc[U1];
    int row1[U1];   // (offsets, not pointers: half the registers)
#pragma unroll
    for (int u = 0; u < U1; u++) {
        const int j = (int)gl + u * G, net = j / kPolH1, jj = j % kPolH1;
        row1[u] = net * L.vf() + L.W1 + jj * D;
        acc[u] = w[net * L.vf() + L.B1 + jj];
    }
#pragma unroll 2
    for (int k = 0; k < D; k++) {
        const float xk = xs[k];
#pragma unroll
        for (int u = 0; u < U1; u++) acc[u] = fmaf(w[row1[u] + k], xk, acc[u]);
    }
    pol_group_sync();   // every lane has read the row: xs takes layer 1's outputs
#pragma unroll
    for (int u = 0; u < U1; u++) xs[(int)gl + u * G] = tanh_fast(acc[u]);
    pol_group_sync();
    // layer 2: unit j = gl + u G of the 32 (pi 0..15, vf 16..31)
    float acc2[U2];
#pragma unroll
    for (int u = 0; u < U2; u++) {
        const int j = (int)gl + u * G, net = j / kPolH2, jj = j % kPolH2;
        const float *W2 = w + net * L.vf() + L.W2, *b2 = w + net * L.vf() + L.B2;
        const float *z1 = xs + net * kPolH1;
        float s = b2[jj];
#pragma unroll 8
        for (int k = 0; k < kPolH1; k++) s = fmaf(W2[jj * kPolH1 + k], z1[k], s);
        acc2[u] = s;
    }
    pol_group_sync();
#pragma unroll
    for (int u = 0; u < U2; u++) xs[(int)gl + u * G] = tanh_fast(acc2[u]);
    pol_group_sync();
    // output: lane 0 the pi head (mean, action, log-probability), lane 1 the value
    if (gl < 2u) {
        const int net = (int)gl;
        const float *W3 = w + net * L.vf() + L.W3, *b3 = w + net * L.vf() + L.B3;
        const float *z2 = xs + net * kPolH2;
        float out = b3[0];
#pragma unroll
        for (int k = 0; k < kPolH2; k++) out = fmaf(W3[k], z2[k], out);
        if (net == 0) {
            const float log_std = w[L.log_std()];
            const float eps = P.noise ? P.noise[(int64_t)t * n + i] : 0.0f;
            P.act[pol_act_row(P, t) * n + i] = gaussian_act(out, log_std, eps);
            if (P.logp) P.logp[(int64_t)t * n + i] = gaussian_logp(eps, log_std);
        } else if (P.value) {
            P.value[(int64_t)t * n + i] = out;
        }
    }
    pol_group_sync();   // (the next use of xs -- the next env or step of this group -- after every lane's reads)
}

}  // namespace pcc
