// pcc_gradclip.hip -- a global gradient-norm limit and a non-finite guard BESIDE the fused PPO step (include/pcc_policy.h:
// pcc_ppo_minibatch_step_clip_pop).  The step's own two launches run untouched as "gradient only" (every
// member's lr = 0 in a work copy of hyper: ppo_adam_kernel writes the summed gradient G and the statistics and returns), and
// what an optimiser step does with G happens here:
//
//   clip_hyper_kernel  one thread per float of hyper: hyper_grad = hyper with column 0 (lr) = 0.
//   clip_adam_kernel   grid (n_members), 256 lanes: lane j adds the float64 squares of G[p], p = j, j + 256, ... in increasing p
//                      (coalesced: a wavefront reads 256 consecutive bytes), the 256 lane sums go through a halving tree in LDS
//                      (s = 128, 64, ..., 1: x[j] += x[j + s] for j < s) -- the order is the contract: the same G gives the same
//                      bits, and a numpy restatement gives them too --, every lane reads sumsq = x[0] and takes the member's state
//                      and coefficient c; then, unless the member is skipped or gradient-only, Adam on G[p] * c, operation for
//                      operation as ppo_adam_kernel (pcc_ppo.hip) does it on G[p]: with c == 1.0f the bits are that kernel's.
//                      Lane 0 writes the member's row of `clip`.
//
// No atomics, no hand-off between workgroups.  A unit of its own (see pcc_obsnorm.hip: adding kernels to an existing unit moves
// the old kernels' schedules): pcc_ppo.hip and the tile units keep their device code instruction for instruction.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pcc_policy.h"
#include "pcc_policy_dev.h"

namespace {

constexpr int kClipThreads = 256;
constexpr int kClipMaxMembers = 1024;
constexpr int kClipHyperCols = 8;   // a row of `hyper`
constexpr int kClipHyperLr = 0;     // ... its learning rate
constexpr int kClipHyperMax = 5;    // ... and the member's limit on the gradient norm (0: the guard alone)
constexpr int kClipCols = 8;        // a row of `clip`
constexpr double kClipEps = 1e-6;   // torch.nn.utils.clip_grad_norm_'s

__global__ __launch_bounds__(kClipThreads) void clip_hyper_kernel(const float *__restrict__ hyper, int n, float *__restrict__ hyper_grad) {
    const int i = blockIdx.x * kClipThreads + threadIdx.x;
    if (i >= n) return;
    hyper_grad[i] = i % kClipHyperCols == kClipHyperLr ? 0.0f : hyper[i];
}

__global__ __launch_bounds__(kClipThreads) void clip_adam_kernel(const float *__restrict__ grad_all, int n_params,
                                                                 const float *__restrict__ hyper, float *__restrict__ params_all,
                                                                 float *__restrict__ m_all, float *__restrict__ v_all,
                                                                 int64_t param_stride, float beta1, float beta2, float eps, float bias1,
                                                                 float bias2_sqrt, double *__restrict__ clip_all, int64_t clip_stride) {
    __shared__ double x[kClipThreads];
    const int tid = threadIdx.x;
    const int64_t mb = blockIdx.x, po = mb * param_stride;
    const float *__restrict__ grad = grad_all + po;
    double acc = 0.0;
#pragma unroll 4
    for (int p = tid; p < n_params; p += kClipThreads) {
        const double g = (double)grad[p];
        acc += g * g;
    }
    x[tid] = acc;
    __syncthreads();
    for (int s = kClipThreads >> 1; s >= 1; s >>= 1) {
        if (tid < s) x[tid] += x[tid + s];
        __syncthreads();
    }
    const double sumsq = x[0], norm = sqrt(sumsq);
    const float lr = hyper[mb * kClipHyperCols + kClipHyperLr], limit = hyper[mb * kClipHyperCols + kClipHyperMax];
    const double c64 = (double)limit / (norm + kClipEps);
    int state = 0;
    float c = 1.0f;
    if (lr == 0.0f) {
        state = 3;   // gradient only
    } else if (!isfinite(sumsq)) {
        state = 2;   // skipped: a NaN or an infinity in G reaches neither the parameters nor the moments
    } else if (limit > 0.0f && c64 < 1.0) {
        state = 1;
        c = (float)c64;
    }
    if (tid == 0) {
        double *row = clip_all + mb * clip_stride;
        row[0] = sumsq;
        row[1] = norm;
        row[2] = (double)c;
        row[3] = (double)state;
        if (state <= 1) row[4] += 1.0;
        if (state == 1) row[5] += 1.0;
        if (state == 2) row[6] += 1.0;
        row[7] = fmax(row[7], norm);   // (a NaN norm does not enter it)
    }
    if (state >= 2) return;
    float *__restrict__ params = params_all + po, *__restrict__ m = m_all + po, *__restrict__ v = v_all + po;
    for (int p = tid; p < n_params; p += kClipThreads) {
        const float g = grad[p] * c;
        // (from here on ppo_adam_kernel's lines, kept in step by hand)
        const float mm = beta1 * m[p] + (1.0f - beta1) * g;
        const float vv = beta2 * v[p] + (1.0f - beta2) * g * g;
        m[p] = mm;
        v[p] = vv;
        const float denom = sqrtf(vv) / bias2_sqrt + eps;
        params[p] -= (lr / bias1) * (mm / denom);
    }
}

}  // namespace

extern "C" int pcc_ppo_minibatch_step_clip_pop(const float *obs, const float *act, const float *logp_old, const float *adv,
                                               const float *ret, const int64_t *perm, int64_t perm_stride, int64_t start,
                                               int64_t count, int obs_dim, int h1, int h2, float *params, float *adam_m, float *adam_v,
                                               int64_t param_stride, int n_members, const float *hyper, int adam_step, float beta1,
                                               float beta2, float eps, float *scratch, float *grad_out, float *stats_out,
                                               float *hyper_grad, double *clip, int64_t clip_stride, void *stream) {
    // pcc_ppo_minibatch_step_pop's refusals, in its order, and this entry's own: all before the first launch (a host without a
    // device gives the same answers)
    if (!obs || !act || !logp_old || !adv || !ret || !perm || !params || !scratch || !hyper || count < 1 || start < 0) return -1;
    if (!adam_m || !adam_v || adam_step < 1) return -1;
    if (n_members < 1 || n_members > kClipMaxMembers || perm_stride < 0) return -1;
    if (!grad_out || !hyper_grad || !clip || clip_stride < kClipCols || hyper_grad == hyper) return -1;
    if (pcc_ppo_supported(obs_dim, h1, h2) != 1) return -2;
    const int n_params = pcc::PolicyLayout(obs_dim, h1, h2).n_params();
    if (param_stride < n_params || param_stride % 64 != 0) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n_hyper = n_members * kClipHyperCols;
    hipLaunchKernelGGL(clip_hyper_kernel, dim3((unsigned)((n_hyper + kClipThreads - 1) / kClipThreads)), dim3(kClipThreads), 0, st, hyper,
                       n_hyper, hyper_grad);
    if (hipGetLastError() != hipSuccess) return -3;
    const int rc = pcc_ppo_minibatch_step_pop(obs, act, logp_old, adv, ret, perm, perm_stride, start, count, obs_dim, h1, h2, params, adam_m,
                                              adam_v, param_stride, n_members, hyper_grad, adam_step, beta1, beta2, eps, scratch, grad_out,
                                              stats_out, stream);
    if (rc != 0) return rc;
    // the bias corrections as launch_step (pcc_ppo.hip) computes them
    const float bias1 = 1.0f - powf(beta1, (float)adam_step);
    const float bias2 = sqrtf(1.0f - powf(beta2, (float)adam_step));
    hipLaunchKernelGGL(clip_adam_kernel, dim3((unsigned)n_members), dim3(kClipThreads), 0, st, grad_out, n_params, hyper, params, adam_m,
                       adam_v, param_stride, beta1, beta2, eps, bias1, bias2, clip, clip_stride);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
