// pcc_policy_dev.h -- the device side of the policy forward that both the stand-alone policy kernel (pcc_policy.hip) and the
// rollout epilogue of the env's kernels (pcc_retire.hip, pcc_small.hip: pcc_rollout) evaluate.  The epilogue must give the
// stand-alone kernel's bits (include/pcc_sim.h: pcc_rollout), so what the two share lives here, once.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcc {

// tanh(x) = 1 - 2 / (exp(2x) + 1) by the hardware's exp2 and reciprocal: absolute error ~1e-7, saturates cleanly -- the same
// function the gradient kernel evaluates (pcc_ppo.hip: the rollout's and the update's forward agree), a fifth of libm's tanhf
// in instructions (48 of them per network and env: half of the fixed kernel's time went into them)
__device__ __forceinline__ float tanh_fast(float x) {
    const float e = __expf(2.0f * x);
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

// The epilogue's network: the reference's --arch 32,16 (pcc_policy_act's fixed kernel), any observation length up to 64.
constexpr int kPolH1 = 32, kPolH2 = 16, kPolMaxObs = 64;
constexpr int kPolScratch = 64;   // LDS floats per env of the epilogue: the observation row, then layer 1's, then layer 2's outputs

__host__ __device__ constexpr int pol_net_floats(int D) { return kPolH1 * D + kPolH1 + kPolH2 * kPolH1 + kPolH2 + kPolH2 + 1; }
__host__ __device__ constexpr int pol_params(int D) { return 2 * pol_net_floats(D) + 1; }   // pi {.., log_std}, vf

// What a launch with the policy in its epilogue computes (pcc_rollout): after its step s (0-based within the launch) the env's
// next action -- the policy on the observation row the step just wrote -- goes to row t0 + s + 1 of act / logp / value, with
// noise row t0 + s + 1 (noise NULL: deterministic).  Rows are [N] (one sender).  act has act_rows rows used round robin
// (0 = a row per step); the small-batch kernel's send part reads its actions from there too (row t0 + s).
struct PolicyArgs {
    const float *params;   // pcc_policy_act's parameter block (include/pcc_policy.h), device
    int n_params;
    int D;                 // observation length (<= kPolMaxObs)
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
    const int n_net = pol_net_floats(D);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the row's stores (other lanes of this group) before its loads
    for (int x = (int)gl; x < D; x += G) xs[x] = obs_row[x];
    pol_group_sync();
    // layer 1: unit j = gl + u G of the 64 (pi 0..31, vf 32..63)
    float acc[U1];
    int row1[U1];   // (offsets, not pointers: half the registers)
#pragma unroll
    for (int u = 0; u < U1; u++) {
        const int j = (int)gl + u * G, net = j / kPolH1, jj = j % kPolH1;
        row1[u] = net * (n_net + 1) + jj * D;
        acc[u] = w[net * (n_net + 1) + kPolH1 * D + jj];
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
        const float *W2 = w + net * (n_net + 1) + kPolH1 * D + kPolH1;
        const float *z1 = xs + net * kPolH1;
        float s = W2[kPolH2 * kPolH1 + jj];
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
        const float *W3 = w + net * (n_net + 1) + kPolH1 * D + kPolH1 + kPolH2 * kPolH1 + kPolH2;
        const float *z2 = xs + net * kPolH2;
        float out = W3[kPolH2];
#pragma unroll
        for (int k = 0; k < kPolH2; k++) out = fmaf(W3[k], z2[k], out);
        if (net == 0) {
            const float log_std = w[n_net];
            const float eps = P.noise ? P.noise[(int64_t)t * n + i] : 0.0f;
            P.act[pol_act_row(P, t) * n + i] = out + expf(log_std) * eps;
            if (P.logp) P.logp[(int64_t)t * n + i] = -0.5f * eps * eps - log_std - 0.918938533204672742f;
        } else if (P.value) {
            P.value[(int64_t)t * n + i] = out;
        }
    }
    pol_group_sync();   // (the next use of xs -- the next env or step of this group -- after every lane's reads)
}

}  // namespace pcc
