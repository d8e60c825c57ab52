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
// Every kernel has a member dimension in its grid: pcc_policy_act is pcc_policy_act_pop with one member (include/pcc_policy.h), and
// both go through launch_policy_act below.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcc_mlp_tiles.h"
#include "pcc_policy.h"
#include "pcc_policy_dev.h"

namespace {

using pcc::PolicyLayout;
using pcc::tanh_fast;   // (shared with the rollout epilogue of the env's kernels, which must give these kernels' bits)

constexpr int kMaxParams = 8192;   // floats of both networks
constexpr int kMaxHidden = 64;

// The reference's own sizes (--arch 32,16) with everything a compile-time constant: the hidden activations stay in
// registers (the generic kernel below indexes z1[j] with a run-time j: LDS), the loops unroll.
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

// Weights straight from the parameter block with compile-time offsets: every lane reads the same address, so the loads are
// scalar (s_load into SGPRs, which the FMAs take as operands) -- no LDS copy, no LDS read per FMA (the first form of this
// kernel staged the parameters in LDS and read one weight per FMA from there: 32 us for 65 536 envs, LDS-issue-bound with one
// wavefront per SIMD).  The two networks of an env run in two lanes of different workgroups (blockIdx.y = 0: pi -> mean,
// action, log-probability; 1: vf -> value): twice the wavefronts, half the chain.
// blockIdx.z = member of a population (one in a stand-alone call): a workgroup of member m sees that member's n rows and
// parameter block through offset pointers, so blockIdx.x / .y cut a member's rows as a stand-alone launch over them does: the
// same operations, the same bits.  The parameter pointer is uniform over a workgroup, so the weights stay scalar loads.
__device__ __forceinline__ const float *member_rows(const float *p, int64_t off) { return p ? p + off : nullptr; }
__device__ __forceinline__ float *member_rows(float *p, int64_t off) { return p ? p + off : nullptr; }

template <int D, int H1, int H2>
__global__ __launch_bounds__(256) void policy_act_fixed_kernel(const float *__restrict__ obs_all, int64_t n,
                                                               const float *__restrict__ params_all, int64_t param_stride,
                                                               const float *__restrict__ noise_all, float *__restrict__ mean_all,
                                                               float *__restrict__ act_all, float *__restrict__ logp_all,
                                                               float *__restrict__ value_all) {
    const int64_t off = (int64_t)blockIdx.z * n;
    const float *__restrict__ obs = obs_all + off * D, *__restrict__ params = params_all + (int64_t)blockIdx.z * param_stride;
    const float *__restrict__ noise = member_rows(noise_all, off);
    float *__restrict__ mean_out = member_rows(mean_all, off), *__restrict__ act_out = member_rows(act_all, off);
    float *__restrict__ logp_out = member_rows(logp_all, off), *__restrict__ value_out = member_rows(value_all, off);
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

// The generic kernel for other policies below 8 192 parameters: one lane per env, both networks one after the other, the parameters
// staged in LDS, libm's tanhf.  One network (p = its first float of the staged block) on one observation row, the hidden
// activations in LDS -- column `threadIdx.x` of [unit][256] arrays: conflict-free -- so that the run-time unit index costs no
// scratch memory.  The arrays are dynamic LDS of (h1 + h2) x 256 floats, sized by the launch: 30 KB at hidden 20, 10 next to the
// 32 KB of parameters (two workgroups per CU), 96 KB at 64, 32.
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

// blockIdx.y = member (one in a stand-alone call), n = a member's rows
template <int D>
__global__ __launch_bounds__(256) void policy_act_kernel(const float *__restrict__ obs, int64_t n,
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
    if (r >= n) return;
    const int64_t i = (int64_t)blockIdx.y * n + r;
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

// The forward of n_members policies on n_envs / n_members rows each (both entry points; the arguments are checked there).
static int launch_policy_act(const pcc_tiles::ActArgs &a, hipStream_t st) {
    const int n_params = PolicyLayout(a.D, a.h1, a.h2).n_params();
    if (n_params > kMaxParams || !pcc::fixed_act_length(a.D))   // what the kernels of this file refuse: the tiled kernel (-2 outside its domain)
        return pcc_tiles::launch_act(a, st);
    const unsigned gx = (unsigned)((a.n + 255) / 256), members = (unsigned)a.n_members;
    const dim3 block(256);
    const bool fixed_net = a.h1 == 32 && a.h2 == 16;   // the reference's --arch: the fully unrolled build
    constexpr int kMaxDynLds = 2 * kMaxHidden * 256 * (int)sizeof(float);   // with the 32 KB of parameters: the 160 KB of a CU
    const unsigned zs_bytes = (unsigned)(a.h1 + a.h2) * 256u * (unsigned)sizeof(float);
    // the observation length is a compile-time constant of both kernels (unrolled loads)
#define PCC_POLICY_CASE(DD)                                                                                                          \
    if (a.D == DD) {                                                                                                                 \
        if (fixed_net)                                                                                                               \
            hipLaunchKernelGGL((policy_act_fixed_kernel<DD, 32, 16>), dim3(gx, 2, members), block, 0, st, a.obs, a.n, a.params,      \
                               a.param_stride, a.noise, a.mean_out, a.act_out, a.logp_out, a.value_out);                            \
        else {                                                                                                                       \
            /* (above 64 KB of dynamic LDS a kernel has to be told so, once) */                                                      \
            static const hipError_t lds_ok = hipFuncSetAttribute(reinterpret_cast<const void *>(&policy_act_kernel<DD>),              \
                                                                 hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynLds);            \
            if (lds_ok != hipSuccess) return -3;                                                                                     \
            hipLaunchKernelGGL(policy_act_kernel<DD>, dim3(gx, members), block, zs_bytes, st, a.obs, a.n, a.params, a.param_stride,  \
                               n_params, a.h1, a.h2, a.noise, a.mean_out, a.act_out, a.logp_out, a.value_out);                      \
        }                                                                                                                            \
    }
    PCC_FIXED_OBS_LENGTHS(PCC_POLICY_CASE)
#undef PCC_POLICY_CASE
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int pcc_policy_act(const float *obs, int64_t n_envs, int obs_dim, const float *params, int h1, int h2,
                              const float *noise, float *mean_out, float *act_out, float *logp_out, float *value_out,
                              void *stream) {
    if (!obs || !params || n_envs < 1) return -1;
    if (h1 < 1 || h2 < 1 || h1 > kMaxHidden || h2 > kMaxHidden) return -1;
    const pcc_tiles::ActArgs a{obs, n_envs, obs_dim, h1, h2, params, 0, 1, noise, mean_out, act_out, logp_out, value_out};
    return launch_policy_act(a, static_cast<hipStream_t>(stream));
}

extern "C" int pcc_policy_act_pop(const float *obs, int64_t n_envs, int obs_dim, const float *params, int64_t param_stride,
                                  int n_members, int h1, int h2, const float *noise, float *mean_out, float *act_out,
                                  float *logp_out, float *value_out, void *stream) {
    if (!obs || !params || n_envs < 1) return -1;
    if (h1 < 1 || h2 < 1 || h1 > kMaxHidden || h2 > kMaxHidden) return -1;
    if (n_members < 1 || n_members > 1024 || n_envs % n_members != 0) return -1;
    if (obs_dim < 1 || obs_dim > 128) return -2;   // (pcc_policy_act's answer, before the stride is held against the layout)
    if (param_stride < PolicyLayout(obs_dim, h1, h2).n_params() || param_stride % 64 != 0) return -1;
    const pcc_tiles::ActArgs a{obs, n_envs / n_members, obs_dim, h1, h2, params, param_stride, n_members, noise, mean_out, act_out,
                               logp_out, value_out};
    return launch_policy_act(a, static_cast<hipStream_t>(stream));
}
