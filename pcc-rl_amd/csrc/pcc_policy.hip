// pcc_policy.hip -- the rollout half of the on-device PPO caller: the
// reference's policy (src/gym/stable_solve.py:39-45: separate pi / vf MLPs, hidden sizes --arch = 32,16,
// tanh, a state-independent log-std Gaussian head) evaluated for a whole env batch in ONE launch --
// action mean, sampled action, its log-probability and the value estimate -- so that the env half is
// not starved by a dozen small framework launches per step.  One lane per env; the few thousand
// parameters sit in LDS, every lane walks them in the same order (broadcast reads, no bank conflicts);
// fp32 like the framework path it replaces.  No MFMA: 65 536 x ~3 kFLOP is microseconds of plain FMAs.
// That holds for the kernels of this file, both built for the observation lengths of PCC_FIXED_OBS_LENGTHS (pcc_policy_dev.h):
// the reference's --arch 32,16 fully unrolled, and the older generic kernel for other policies below 8 192 parameters.  Every
// other shape of the supported domain (up to 128 observations, hidden layers up to 64 wide, run-time sizes) takes
// policy_act_tiled_kernel (pcc_mlp_tiles.h): the gradient kernel's MFMA forward, weights and activations in LDS, no private
// arrays.  The parameter block's layout, tanh_fast and the Gaussian head are pcc_policy_dev.h's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcc_mlp_tiles_pop.h"
#include "pcc_policy.h"
#include "pcc_policy_dev.h"

namespace {

using pcc::PolicyLayout;
using pcc::tanh_fast;   // (shared with the rollout epilogue of the env's kernels, which must give these kernels' bits)

constexpr int kMaxParams = 8192;   // floats of both networks
constexpr int kMaxHidden = 64;

// one network (p = its first float of the parameter block) on one observation row.  The pointers are chained as they always
// were, not taken from PolicyLayout's offsets: with run-time sizes that folds the address arithmetic differently and changes this
// old kernel's register counts (policy_act_kernel<3>: 38 -> 36 scalar registers) -- it is left as it was generated.
__device__ __forceinline__ float mlp_forward(const float *p, const float *x, int D, int h1, int h2, float *z1, float *z2) {
    const float *W1 = p, *b1 = W1 + h1 * D, *W2 = b1 + h1, *b2 = W2 + h2 * h1, *W3 = b2 + h2, *b3 = W3 + h2;
    for (int j = 0; j < h1; j++) {
        float s = b1[j];
        for (int k = 0; k < D; k++) s = fmaf(W1[j * D + k], x[k], s);
        z1[j] = tanhf(s);
    }
    for (int j = 0; j < h2; j++) {
        float s = b2[j];
        for (int k = 0; k < h1; k++) s = fmaf(W2[j * h1 + k], z1[k], s);
        z2[j] = tanhf(s);
    }
    float out = b3[0];
    for (int k = 0; k < h2; k++) out = fmaf(W3[k], z2[k], out);
    return out;
}

template <int D>
__global__ __launch_bounds__(256) void policy_act_kernel(const float *obs, int64_t n, const float *params, int n_params,
                                                         int h1, int h2, const float *noise, float *mean_out,
                                                         float *act_out, float *logp_out, float *value_out) {
    __shared__ float sp[kMaxParams];
    for (int k = threadIdx.x; k < n_params; k += blockDim.x) sp[k] = params[k];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x[D];
#pragma unroll
    for (int k = 0; k < D; k++) x[k] = obs[i * D + k];
    float z1[kMaxHidden], z2[kMaxHidden];
    const float mu = mlp_forward(sp, x, D, h1, h2, z1, z2);
    const PolicyLayout L(D, h1, h2);   // (after the first forward: placed above it, this old kernel's scalar code moves)
    const float log_std = sp[L.log_std()];
    const float v = mlp_forward(sp + L.vf(), x, D, h1, h2, z1, z2);
    const float eps = noise ? noise[i] : 0.0f;
    const float a = pcc::gaussian_act(mu, log_std, eps);
    if (mean_out) mean_out[i] = mu;
    if (act_out) act_out[i] = a;
    if (logp_out) logp_out[i] = pcc::gaussian_logp(eps, log_std);
    if (value_out) value_out[i] = v;
}

// The reference's own sizes (--arch 32,16) with everything a compile-time constant: the hidden activations stay in
// registers (the generic kernel above indexes z1[j] with a run-time j: scratch memory), the loops unroll.
template <int D, int H1, int H2>
__device__ __forceinline__ float mlp_forward_fixed(const float *p, const float (&x)[D]) {
    constexpr PolicyLayout L(D, H1, H2);
    const float *W1 = p + L.W1, *b1 = p + L.B1, *W2 = p + L.W2, *b2 = p + L.B2, *W3 = p + L.W3, *b3 = p + L.B3;
    float z1[H1], z2[H2];
#pragma unroll
    for (int j = 0; j < H1; j++) {
        float s = b1[j];
#pragma unroll
        for (int k = 0; k < D; k++) s = fmaf(W1[j * D + k], x[k], s);
        z1[j] = tanh_fast(s);
    }
#pragma unroll
    for (int j = 0; j < H2; j++) {
        float s = b2[j];
#pragma unroll
        for (int k = 0; k < H1; k++) s = fmaf(W2[j * H1 + k], z1[k], s);
        z2[j] = tanh_fast(s);
    }
    float out = b3[0];
#pragma unroll
    for (int k = 0; k < H2; k++) out = fmaf(W3[k], z2[k], out);
    return out;
}

// policy_act_fixed_kernel's statements (below) as the body of its population twin, policy_act_fixed_pop_kernel: a copy, kept in
// step by hand and held against the original bit for bit by tests/test_population.py -- called from the old kernel too, the body
// moves that kernel's code.
template <int D, int H1, int H2>
__device__ __forceinline__ void policy_act_fixed_body(const float *__restrict__ obs, int64_t n, const float *__restrict__ params, const float *__restrict__ noise,
                                                      float *__restrict__ mean_out, float *__restrict__ act_out, float *__restrict__ logp_out, float *__restrict__ value_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x[D];
#pragma unroll
    for (int k = 0; k < D; k++) x[k] = obs[i * D + k];
    constexpr PolicyLayout L(D, H1, H2);
    if (blockIdx.y == 0) {
        const float mu = mlp_forward_fixed<D, H1, H2>(params, x);
        const float log_std = params[L.log_std()];
        const float eps = noise ? noise[i] : 0.0f;
        if (mean_out) mean_out[i] = mu;
        if (act_out) act_out[i] = pcc::gaussian_act(mu, log_std, eps);
        if (logp_out) logp_out[i] = pcc::gaussian_logp(eps, log_std);
    } else {
        const float v = mlp_forward_fixed<D, H1, H2>(params + L.vf(), x);
        if (value_out) value_out[i] = v;
    }
}

// Weights straight from the parameter block with compile-time offsets: every lane reads the same address, so the loads are
// scalar (s_load into SGPRs, which the FMAs take as operands) -- no LDS copy, no LDS read per FMA (the first form of this
// kernel staged the parameters in LDS and read one weight per FMA from there: 32 us for 65 536 envs, LDS-issue-bound with one
// wavefront per SIMD).  The two networks of an env run in two lanes of different workgroups (blockIdx.y = 0: pi -> mean,
// action, log-probability; 1: vf -> value): twice the wavefronts, half the chain.
template <int D, int H1, int H2>
__global__ __launch_bounds__(256) void policy_act_fixed_kernel(const float *__restrict__ obs, int64_t n,
                                                               const float *__restrict__ params, int n_params,
                                                               const float *__restrict__ noise, float *__restrict__ mean_out,
                                                               float *__restrict__ act_out, float *__restrict__ logp_out,
                                                               float *__restrict__ value_out) {
    (void)n_params;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x[D];
#pragma unroll
    for (int k = 0; k < D; k++) x[k] = obs[i * D + k];
    constexpr PolicyLayout L(D, H1, H2);
    if (blockIdx.y == 0) {
        const float mu = mlp_forward_fixed<D, H1, H2>(params, x);
        const float log_std = params[L.log_std()];
        const float eps = noise ? noise[i] : 0.0f;
        if (mean_out) mean_out[i] = mu;
        if (act_out) act_out[i] = pcc::gaussian_act(mu, log_std, eps);
        if (logp_out) logp_out[i] = pcc::gaussian_logp(eps, log_std);
    } else {
        const float v = mlp_forward_fixed<D, H1, H2>(params + L.vf(), x);
        if (value_out) value_out[i] = v;
    }
}

// ---- the population forward (pcc_policy_act_pop): the member is one more grid dimension.  A workgroup of member m sees that
// member's rows and parameter block through offset pointers and runs the body of the stand-alone kernel with n = the member's
// rows: the same decomposition (blockIdx.x / .y mean what they mean there), the same operations, the same bits.  The parameter
// pointer is uniform over a workgroup, so the fixed kernel's weights stay scalar loads.
__device__ __forceinline__ const float *member_rows(const float *p, int64_t off) { return p ? p + off : nullptr; }
__device__ __forceinline__ float *member_rows(float *p, int64_t off) { return p ? p + off : nullptr; }

template <int D, int H1, int H2>
__global__ __launch_bounds__(256) void policy_act_fixed_pop_kernel(const float *__restrict__ obs, int64_t n_member,
                                                                   const float *__restrict__ params, int64_t param_stride,
                                                                   const float *__restrict__ noise, float *__restrict__ mean_out,
                                                                   float *__restrict__ act_out, float *__restrict__ logp_out,
                                                                   float *__restrict__ value_out) {
    const int64_t off = (int64_t)blockIdx.z * n_member;
    policy_act_fixed_body<D, H1, H2>(obs + off * D, n_member, params + (int64_t)blockIdx.z * param_stride, member_rows(noise, off),
                                     member_rows(mean_out, off), member_rows(act_out, off), member_rows(logp_out, off),
                                     member_rows(value_out, off));
}

// The older generic kernel for a population: policy_act_kernel's operations in its order (mlp_forward's fmaf chains and tanhf),
// with the hidden activations in LDS -- column `threadIdx.x` of [unit][256] arrays: conflict-free -- instead of private arrays
// indexed at run time, so that this kernel has no scratch memory.  The arrays are dynamic LDS of (h1 + h2) x 256 floats, sized by
// the launch: 30 KB at hidden 20, 10 next to the 32 KB of parameters (two workgroups per CU), 128 KB at 64, 64.  blockIdx.y = member.
__device__ __forceinline__ float mlp_forward_lds(const float *p, const float *x, int D, int h1, int h2, float *z1, float *z2) {
    const float *W1 = p, *b1 = W1 + h1 * D, *W2 = b1 + h1, *b2 = W2 + h2 * h1, *W3 = b2 + h2, *b3 = W3 + h2;
    for (int j = 0; j < h1; j++) {
        float s = b1[j];
        for (int k = 0; k < D; k++) s = fmaf(W1[j * D + k], x[k], s);
        z1[j * 256] = tanhf(s);
    }
    for (int j = 0; j < h2; j++) {
        float s = b2[j];
        for (int k = 0; k < h1; k++) s = fmaf(W2[j * h1 + k], z1[k * 256], s);
        z2[j * 256] = tanhf(s);
    }
    float out = b3[0];
    for (int k = 0; k < h2; k++) out = fmaf(W3[k], z2[k * 256], out);
    return out;
}

template <int D>
__global__ __launch_bounds__(256) void policy_act_pop_kernel(const float *__restrict__ obs, int64_t n_member,
                                                             const float *__restrict__ params_all, int64_t param_stride, int n_params,
                                                             int h1, int h2, const float *__restrict__ noise,
                                                             float *__restrict__ mean_out, float *__restrict__ act_out,
                                                             float *__restrict__ logp_out, float *__restrict__ value_out) {
    __shared__ float sp[kMaxParams];
    extern __shared__ float zs[];   // [h1 + h2][256]
    const float *params = params_all + (int64_t)blockIdx.y * param_stride;
    for (int k = threadIdx.x; k < n_params; k += blockDim.x) sp[k] = params[k];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_member) return;
    const int64_t i = (int64_t)blockIdx.y * n_member + r;
    float x[D];
#pragma unroll
    for (int k = 0; k < D; k++) x[k] = obs[i * D + k];
    float *z1 = zs + threadIdx.x, *z2 = z1 + h1 * 256;
    const float mu = mlp_forward_lds(sp, x, D, h1, h2, z1, z2);
    const PolicyLayout L(D, h1, h2);
    const float log_std = sp[L.log_std()];
    const float v = mlp_forward_lds(sp + L.vf(), x, D, h1, h2, z1, z2);
    const float eps = noise ? noise[i] : 0.0f;
    const float a = pcc::gaussian_act(mu, log_std, eps);
    if (mean_out) mean_out[i] = mu;
    if (act_out) act_out[i] = a;
    if (logp_out) logp_out[i] = pcc::gaussian_logp(eps, log_std);
    if (value_out) value_out[i] = v;
}

}  // namespace

extern "C" int pcc_policy_act(const float *obs, int64_t n_envs, int obs_dim, const float *params, int h1, int h2,
                              const float *noise, float *mean_out, float *act_out, float *logp_out, float *value_out,
                              void *stream) {
    if (!obs || !params || n_envs < 1) return -1;
    if (h1 < 1 || h2 < 1 || h1 > kMaxHidden || h2 > kMaxHidden) return -1;
    const int n_params = PolicyLayout(obs_dim, h1, h2).n_params();
    if (n_params > kMaxParams || !pcc::fixed_act_length(obs_dim)) {   // what the kernels of this file refuse: the tiled kernel (-2 outside its domain)
        const pcc_tiles::ActArgs a{obs, n_envs, obs_dim, h1, h2, params, noise, mean_out, act_out, logp_out, value_out};
        return pcc_tiles::launch_act(a, static_cast<hipStream_t>(stream));
    }
    const dim3 grid((unsigned)((n_envs + 255) / 256)), block(256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool fixed_net = h1 == 32 && h2 == 16;   // the reference's --arch: the fully unrolled build
    // the observation length is a compile-time constant of both kernels (unrolled loads)
#define PCC_POLICY_CASE(DD)                                                                                                          \
    if (obs_dim == DD) {                                                                                                             \
        if (fixed_net)                                                                                                               \
            hipLaunchKernelGGL((policy_act_fixed_kernel<DD, 32, 16>), dim3(grid.x, 2), block, 0, st, obs, n_envs, params, n_params, noise, \
                               mean_out, act_out, logp_out, value_out);                                                             \
        else                                                                                                                         \
            hipLaunchKernelGGL(policy_act_kernel<DD>, grid, block, 0, st, obs, n_envs, params, n_params, h1, h2, noise, mean_out,    \
                               act_out, logp_out, value_out);                                                                       \
    }
    PCC_FIXED_OBS_LENGTHS(PCC_POLICY_CASE)
#undef PCC_POLICY_CASE
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int pcc_policy_act_pop(const float *obs, int64_t n_envs, int obs_dim, const float *params, int64_t param_stride,
                                  int n_members, int h1, int h2, const float *noise, float *mean_out, float *act_out,
                                  float *logp_out, float *value_out, void *stream) {
    if (!obs || !params || n_envs < 1) return -1;
    if (h1 < 1 || h2 < 1 || h1 > kMaxHidden || h2 > kMaxHidden) return -1;
    if (n_members < 1 || n_members > 1024 || n_envs % n_members != 0) return -1;
    if (obs_dim < 1 || obs_dim > 128) return -2;   // (pcc_policy_act's answer, before the stride is held against the layout)
    const int n_params = PolicyLayout(obs_dim, h1, h2).n_params();
    if (param_stride < n_params || param_stride % 64 != 0) return -1;
    const int64_t n_member = n_envs / n_members;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_params > kMaxParams || !pcc::fixed_act_length(obs_dim)) {   // as in pcc_policy_act: the tiled kernel (-2 outside its domain)
        const pcc_tiles::ActPopArgs a{{obs, n_member, obs_dim, h1, h2, params, noise, mean_out, act_out, logp_out, value_out},
                                      param_stride, n_members};
        return pcc_tiles::launch_act_pop(a, st);
    }
    const unsigned gx = (unsigned)((n_member + 255) / 256);   // a member's rows as a stand-alone launch cuts them
    const dim3 block(256);
    const bool fixed_net = h1 == 32 && h2 == 16;
    constexpr int kPopMaxDynLds = 2 * kMaxHidden * 256 * (int)sizeof(float);   // with the 32 KB of parameters: the 160 KB of a CU
    const unsigned zs_bytes = (unsigned)(h1 + h2) * 256u * (unsigned)sizeof(float);
#define PCC_POLICY_CASE(DD)                                                                                                          \
    if (obs_dim == DD) {                                                                                                             \
        if (fixed_net)                                                                                                               \
            hipLaunchKernelGGL((policy_act_fixed_pop_kernel<DD, 32, 16>), dim3(gx, 2, (unsigned)n_members), block, 0, st, obs, n_member, \
                               params, param_stride, noise, mean_out, act_out, logp_out, value_out);                                \
        else {                                                                                                                       \
            /* (above 64 KB of dynamic LDS a kernel has to be told so, once) */                                                      \
            static const hipError_t lds_ok = hipFuncSetAttribute(reinterpret_cast<const void *>(&policy_act_pop_kernel<DD>),          \
                                                                 hipFuncAttributeMaxDynamicSharedMemorySize, kPopMaxDynLds);         \
            if (lds_ok != hipSuccess) return -3;                                                                                     \
            hipLaunchKernelGGL(policy_act_pop_kernel<DD>, dim3(gx, (unsigned)n_members), block, zs_bytes, st, obs, n_member, params, \
                               param_stride, n_params, h1, h2, noise, mean_out, act_out, logp_out, value_out);                      \
        }                                                                                                                            \
    }
    PCC_FIXED_OBS_LENGTHS(PCC_POLICY_CASE)
#undef PCC_POLICY_CASE
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
