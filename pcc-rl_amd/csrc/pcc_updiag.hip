// pcc_updiag.hip -- what an update did to the policy, and the KL guard: per member the approximate KL divergence between the
// rollout's policy and the updated one, the clip fraction over the whole rollout and the explained variance of the value function,
// from the [T][n_envs] rows a rollout already holds and the updated policy's means; and the per-member decision to stop updating,
// taken on the device (include/pcc_policy.h: pcc_policy_act_rows_pop, pcc_update_diag_pop and its stand-alone form; DESIGN.md
// section 23).
//
//   diag_walk_kernel   grid (G, n_members), 256 threads, G = ceil(n_m / 256): lane = env, member-local index blockIdx.x * 256 + tid
//                      (a member is cut into workgroups exactly as a launch over the member alone).  The lane walks the rows t = 0,
//                      row_step, 2 row_step, ... < T in this order: five coalesced float32 loads per sample (20 bytes), four rows'
//                      loads issued before the dependent chains.  Per sample the float32 log-ratio d32 as the header states it,
//                      then in float64 k = expm1(d) - d, the clip test, the non-finite test and fmax(|d|).  A lane carries the sum
//                      of k, two exact counters, the maximum, and for ret and for e = ret - val ONE float64 pair {sum, sum of
//                      squares} of x - x0, x0 the lane's first sample (pcc_rewnorm.hip's form: no cancellation against a large mean,
//                      no division per sample), which gives the lane's {mean, m2}.  The lanes of a wavefront are combined in a
//                      down-shuffle tree (lane 0 holds the result: sums add, the maximum follows fmax, the moments Chan's formula),
//                      the 4 wavefronts through LDS in index order, and the workgroup's kDiagPart doubles go to
//                      scratch[member][workgroup][kDiagPart].
//   diag_merge_kernel  grid (n_members), 256 threads: sub-lane tid combines a contiguous range of the member's partials in index
//                      order -- plain sums, fmax, and for the two moments count-weighted sums of the partial means' distances from
//                      partial 0's and of their squares, no division per partial -- a fixed halving tree in LDS combines the
//                      sub-lanes, and thread 0 writes the member's row of diag, takes the stop decision and writes the member's row
//                      of hyper_live.
//
// An idle lane of a member's last workgroup contributes {count 0, sums 0, maximum 0}: chan_merge leaves the other side as it is.
// No atomics, no hand-off between workgroups: the same inputs give the same bits.  A unit of its own (see pcc_obsnorm.hip: adding
// kernels to an existing unit moves the old kernels' schedules); pcc_policy_act_rows_pop lives here for the same reason and launches
// nothing of its own: it calls pcc_policy_act_pop.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pcc_policy.h"
#include "pcc_policy_dev.h"

namespace {

constexpr int kDiagThreads = 256;
constexpr int kDiagMaxMembers = 1024;
constexpr int kDiagUnroll = 4;       // rows whose loads are in flight together (5 loads each)
constexpr int kDiagHyperCols = 8;    // a row of `hyper`
constexpr int kDiagHyperClip = 1;    // ... and the column ppo_grad_* read the clip range from
constexpr int kDiagCols = 8;         // a row of `diag`
// a workgroup's partial: {count, sum k, clipped, nonfinite, max |d|, mean ret, m2 ret, mean e, m2 e}
constexpr int kDiagPart = 9;

// Chan et al.'s pairwise update of two means and two m2 that share their counts: (na; ma, qa; ea, fa) takes (nb; ...) in; an
// empty side leaves the other as it is.  na is NOT updated: the caller adds the counts once.
__device__ __forceinline__ void chan_merge2(double na, double &ma, double &qa, double &ea, double &fa, double nb, double mb, double qb,
                                            double eb, double fb) {
    if (nb == 0.0) return;
    if (na == 0.0) {
        ma = mb; qa = qb; ea = eb; fa = fb;
        return;
    }
    const double n = na + nb, w = na * nb / n, d = mb - ma, g = eb - ea;
    ma = ma + d * nb / n;
    qa = qa + qb + d * d * w;
    ea = ea + g * nb / n;
    fa = fa + fb + g * g * w;
}

__global__ __launch_bounds__(kDiagThreads) void diag_walk_kernel(const float *__restrict__ act, const float *__restrict__ logp_old,
                                                                 const float *__restrict__ mean_new, const float *__restrict__ ret,
                                                                 const float *__restrict__ val, int T, int row_step, int64_t n_envs,
                                                                 int64_t n_m, const float *__restrict__ params, int64_t param_stride,
                                                                 int64_t log_std_index, const float *__restrict__ hyper, float clip_arg,
                                                                 double *__restrict__ scratch) {
    __shared__ double s_part[kDiagThreads / 64][kDiagPart];
    const int tid = threadIdx.x;
    const int64_t local = (int64_t)blockIdx.x * kDiagThreads + tid;
    const bool live = local < n_m;
    const int64_t i = (int64_t)blockIdx.y * n_m + local;   // the env
    const float log_std = params[(int64_t)blockIdx.y * param_stride + log_std_index];
    const float inv = expf(-log_std);
    const double clip = (double)(hyper ? hyper[(int64_t)blockIdx.y * kDiagHyperCols + kDiagHyperClip] : clip_arg);

    double cnt = 0.0, sum_k = 0.0, n_clip = 0.0, n_bad = 0.0, d_max = 0.0, r_mean = 0.0, r_m2 = 0.0, e_mean = 0.0, e_m2 = 0.0;
    if (live) {
        int clipped = 0, bad = 0, rows = 0;
        double r0 = 0.0, rs = 0.0, rq = 0.0, e0 = 0.0, es = 0.0, eq = 0.0;
        // one sample: the float32 log-ratio, then float64
        auto sample = [&](float a, float lo, float mu, float rt, float vl) {
            const float z = (a - mu) * inv;
            const float lp = pcc::gaussian_logp(z, log_std);
            const float d32 = lp - lo;
            const double d = (double)d32;
            const double r1 = expm1(d);
            sum_k += r1 - d;
            clipped += fabs(r1) > clip ? 1 : 0;
            bad += isfinite(d) ? 0 : 1;
            d_max = fmax(d_max, fabs(d));
            const double r = (double)rt, e = (double)rt - (double)vl;
            if (rows == 0) {
                r0 = r; e0 = e;
            }
            const double x = r - r0, y = e - e0;
            rs += x; rq += x * x;
            es += y; eq += y * y;
            rows++;
        };
        const float *ap = act + i, *lp_ = logp_old + i, *mp = mean_new + i, *rp = ret + i, *vp = val + i;
        const int64_t step = (int64_t)row_step * n_envs;   // floats between two selected rows
        const int n_rows = (T - 1) / row_step + 1;
        int j = 0;
        int64_t at = 0;
        for (; j + kDiagUnroll <= n_rows; j += kDiagUnroll) {
            float a[kDiagUnroll], lo[kDiagUnroll], mu[kDiagUnroll], rt[kDiagUnroll], vl[kDiagUnroll];
#pragma unroll
            for (int u = 0; u < kDiagUnroll; u++) {
                const int64_t k = at + (int64_t)u * step;
                a[u] = ap[k]; lo[u] = lp_[k]; mu[u] = mp[k]; rt[u] = rp[k]; vl[u] = vp[k];
            }
#pragma unroll
            for (int u = 0; u < kDiagUnroll; u++) sample(a[u], lo[u], mu[u], rt[u], vl[u]);
            at += (int64_t)kDiagUnroll * step;
        }
        for (; j < n_rows; j++, at += step) sample(ap[at], lp_[at], mp[at], rp[at], vp[at]);
        cnt = (double)rows;
        n_clip = (double)clipped;
        n_bad = (double)bad;
        r_mean = r0 + rs / cnt;
        e_mean = e0 + es / cnt;
        const double rdev = rq - rs * rs / cnt, edev = eq - es * es / cnt;
        r_m2 = rdev > 0.0 ? rdev : 0.0;   // (sums of squared deviations: rounding must not make them negative)
        e_m2 = edev > 0.0 ? edev : 0.0;
    }

    // the wavefront's lanes in a down-shuffle tree: lane 0 ends with the wavefront's values (what the other lanes hold is not used)
    for (int o = 32; o >= 1; o >>= 1) {
        const double nb = __shfl_down(cnt, o), mb = __shfl_down(r_mean, o), qb = __shfl_down(r_m2, o);
        const double eb = __shfl_down(e_mean, o), fb = __shfl_down(e_m2, o);
        chan_merge2(cnt, r_mean, r_m2, e_mean, e_m2, nb, mb, qb, eb, fb);
        cnt += nb;
        sum_k += __shfl_down(sum_k, o);
        n_clip += __shfl_down(n_clip, o);
        n_bad += __shfl_down(n_bad, o);
        d_max = fmax(d_max, __shfl_down(d_max, o));
    }
    if ((tid & 63) == 0) {
        double *w = s_part[tid >> 6];
        w[0] = cnt; w[1] = sum_k; w[2] = n_clip; w[3] = n_bad; w[4] = d_max; w[5] = r_mean; w[6] = r_m2; w[7] = e_mean; w[8] = e_m2;
    }
    __syncthreads();
    if (tid == 0) {   // ... then the 4 wavefronts in index order
        for (int v = 1; v < kDiagThreads / 64; v++) {
            const double *w = s_part[v];
            chan_merge2(cnt, r_mean, r_m2, e_mean, e_m2, w[0], w[5], w[6], w[7], w[8]);
            cnt += w[0]; sum_k += w[1]; n_clip += w[2]; n_bad += w[3];
            d_max = fmax(d_max, w[4]);
        }
        double *out = scratch + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kDiagPart;
        out[0] = cnt; out[1] = sum_k; out[2] = n_clip; out[3] = n_bad; out[4] = d_max; out[5] = r_mean; out[6] = r_m2; out[7] = e_mean;
        out[8] = e_m2;
    }
}

constexpr int kDiagSums = 11;   // what a sub-lane of the merge carries: 10 sums and the maximum

__global__ __launch_bounds__(kDiagThreads) void diag_merge_kernel(const double *__restrict__ scratch, int groups,
                                                                  const float *__restrict__ hyper, double kl_limit, int epoch,
                                                                  double *__restrict__ diag, int64_t diag_stride,
                                                                  int32_t *__restrict__ stop, float *__restrict__ hyper_live) {
    __shared__ double s_red[kDiagSums][kDiagThreads];
    const int tid = threadIdx.x;
    const double *part = scratch + (int64_t)blockIdx.x * groups * kDiagPart;
    const int per = (groups + kDiagThreads - 1) / kDiagThreads;
    const int g0 = tid * per < groups ? tid * per : groups, g1 = g0 + per < groups ? g0 + per : groups;
    // The member's moments from the partials' {count, mean, m2} in one pass in index order, no division per partial: with d_g the
    // distance of partial g's mean from partial 0's, mean = k + sum(count_g d_g) / n and m2 = sum(m2_g) + sum(count_g d_g^2) -
    // sum(count_g d_g)^2 / n.  (Every partial of a member holds at least one env and one row: no count is 0.)
    const double kr = part[5], ke = part[7];
    double a[kDiagSums];
#pragma unroll
    for (int j = 0; j < kDiagSums; j++) a[j] = 0.0;
    for (int g = g0; g < g1; g++) {
        const double *p = part + (int64_t)g * kDiagPart;
        const double c = p[0], dr = p[5] - kr, de = p[7] - ke;
        a[0] += c; a[1] += p[1]; a[2] += p[2]; a[3] += p[3];
        a[4] += c * dr; a[5] += c * (dr * dr); a[6] += p[6];
        a[7] += c * de; a[8] += c * (de * de); a[9] += p[8];
        a[10] = fmax(a[10], p[4]);
    }
#pragma unroll
    for (int j = 0; j < kDiagSums; j++) s_red[j][tid] = a[j];
    __syncthreads();
    for (int half = kDiagThreads >> 1; half >= 1; half >>= 1) {   // a fixed tree over the sub-lanes
        if (tid < half) {
#pragma unroll
            for (int j = 0; j < kDiagSums - 1; j++) s_red[j][tid] += s_red[j][tid + half];
            s_red[kDiagSums - 1][tid] = fmax(s_red[kDiagSums - 1][tid], s_red[kDiagSums - 1][tid + half]);
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const int m = blockIdx.x;
    const double n = s_red[0][0];
    const double r_between = s_red[5][0] - s_red[4][0] * s_red[4][0] / n, e_between = s_red[8][0] - s_red[7][0] * s_red[7][0] / n;
    const double var_ret = (s_red[6][0] + (r_between > 0.0 ? r_between : 0.0)) / n;
    const double var_resid = (s_red[9][0] + (e_between > 0.0 ? e_between : 0.0)) / n;
    const double approx_kl = s_red[1][0] / n;
    double *row = diag + (int64_t)m * diag_stride;
    row[0] = n;
    row[1] = approx_kl;
    row[2] = s_red[2][0] / n;
    row[3] = var_ret == 0.0 ? (double)NAN : 1.0 - var_resid / var_ret;
    row[4] = s_red[10][0];
    row[5] = var_ret;
    row[6] = var_resid;
    row[7] = s_red[3][0];
    if (!stop) return;
    int32_t s = stop[m];
    if (s == 0 && kl_limit > 0.0 && !(approx_kl <= kl_limit)) {   // (a NaN KL stops the member)
        s = epoch;
        stop[m] = s;
    }
    const float *h = hyper + (int64_t)m * kDiagHyperCols;
    float *hl = hyper_live + (int64_t)m * kDiagHyperCols;
    hl[0] = s != 0 ? 0.0f : h[0];
#pragma unroll
    for (int c = 1; c < kDiagHyperCols; c++) hl[c] = h[c];
}

// the member's workgroups of the walk; -1 outside the domain (no index of the kernels overflows inside it)
int64_t diag_groups(int T, int row_step, int64_t n_envs, int n_members) {
    if (T < 1 || row_step < 1 || n_envs < 1 || n_members < 1 || n_members > kDiagMaxMembers || n_envs % n_members != 0) return -1;
    if (n_envs > INT64_MAX / (int64_t)sizeof(double) / T / 2) return -1;   // (t * n_envs, one row_step past the last row included)
    if (row_step > 1 && n_envs > INT64_MAX / (int64_t)sizeof(double) / row_step / 8) return -1;
    const int64_t groups = (n_envs / n_members + kDiagThreads - 1) / kDiagThreads;
    if (groups > 0x7fffffff / (kDiagPart * (int64_t)n_members)) return -1;
    return groups;
}

int update_diag(const float *act, const float *logp_old, const float *mean_new, const float *ret, const float *val, int T, int row_step,
                int64_t n_envs, int n_members, const float *params, int64_t param_stride, int64_t log_std_index, const float *hyper,
                float clip, double kl_limit, int epoch, double *diag, int64_t diag_stride, int32_t *stop, float *hyper_live,
                double *scratch, void *stream) {
    // (every refusal comes before any HIP call: a host without a device gives the same answers)
    if (!act || !logp_old || !mean_new || !ret || !val || !params || !diag || !scratch) return -1;
    if ((stop == nullptr) != (hyper_live == nullptr)) return -1;
    const int64_t groups = diag_groups(T, row_step, n_envs, n_members);
    if (groups < 0 || diag_stride < kDiagCols || epoch < 1) return -1;
    if (param_stride < 1 || param_stride % 64 != 0 || log_std_index < 0 || log_std_index >= param_stride) return -1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(diag_walk_kernel, dim3((unsigned)groups, (unsigned)n_members), dim3(kDiagThreads), 0, st, act, logp_old, mean_new,
                       ret, val, T, row_step, n_envs, n_envs / n_members, params, param_stride, log_std_index, hyper, clip, scratch);
    if (hipGetLastError() != hipSuccess) return -3;
    hipLaunchKernelGGL(diag_merge_kernel, dim3((unsigned)n_members), dim3(kDiagThreads), 0, st, scratch, (int)groups, hyper, kl_limit,
                       epoch, diag, diag_stride, stop, hyper_live);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

extern "C" int pcc_update_diag_scratch_doubles(int T, int row_step, int64_t n_envs, int n_members) {
    const int64_t groups = diag_groups(T, row_step, n_envs, n_members);
    return groups < 0 ? -1 : (int)(groups * n_members * kDiagPart);
}

extern "C" int pcc_update_diag_pop(const float *act, const float *logp_old, const float *mean_new, const float *ret, const float *val,
                                   int T, int row_step, int64_t n_envs, int n_members, const float *params, int64_t param_stride,
                                   int64_t log_std_index, const float *hyper, double kl_limit, int epoch, double *diag,
                                   int64_t diag_stride, int32_t *stop, float *hyper_live, double *scratch, void *stream) {
    if (!hyper) return -1;
    return update_diag(act, logp_old, mean_new, ret, val, T, row_step, n_envs, n_members, params, param_stride, log_std_index, hyper,
                       0.0f, kl_limit, epoch, diag, diag_stride, stop, hyper_live, scratch, stream);
}

// The stand-alone form: a population of one (no twin kernels); clip comes as an argument, not from hyper, and
// there is no decision to take.
extern "C" int pcc_update_diag(const float *act, const float *logp_old, const float *mean_new, const float *ret, const float *val, int T,
                               int row_step, int64_t n_envs, const float *params, int64_t log_std_index, float clip, double *diag,
                               double *scratch, void *stream) {
    if (log_std_index < 0 || log_std_index > INT64_MAX - 64) return -1;
    return update_diag(act, logp_old, mean_new, ret, val, T, row_step, n_envs, 1, params, (log_std_index / 64 + 1) * 64, log_std_index,
                       nullptr, clip, 0.0, 1, diag, kDiagCols, nullptr, nullptr, scratch, stream);
}

// The deterministic forward of pcc_policy_act_pop on the rows t = 0, row_step, ... < T of obs[T][n_envs][obs_dim]: one library call,
// the launches are pcc_policy_act_pop's own, one per row, so the bits are its bits.  With ONE member and every row selected the T
// rows are one batch of T * n_envs envs and one launch: every policy kernel computes a row's outputs from that row and the weights
// alone (a lane per env, or a tile's MFMA columns), so where a row sits in the grid does not change its bits
// (tests/test_update_diag.py holds both forms against the row-by-row calls).  pcc_policy_act_pop's argument checks are repeated here
// so that every refusal comes before the first launch.
extern "C" int pcc_policy_act_rows_pop(const float *obs, int T, int row_step, int64_t n_envs, int obs_dim, const float *params,
                                       int64_t param_stride, int n_members, int h1, int h2, float *mean_out, float *value_out,
                                       void *stream) {
    if (T < 1 || row_step < 1) return -1;
    if (!obs || !params || n_envs < 1) return -1;
    if (h1 < 1 || h2 < 1 || h1 > 64 || h2 > 64) return -1;
    if (n_members < 1 || n_members > 1024 || n_envs % n_members != 0) return -1;
    if (obs_dim < 1 || obs_dim > 128) return -2;
    if (param_stride < pcc::PolicyLayout(obs_dim, h1, h2).n_params() || param_stride % 64 != 0) return -1;
    if (n_envs > INT64_MAX / (int64_t)sizeof(float) / obs_dim / T) return -1;
    // launch_policy_act's grids over n rows: ceil(n / 256) workgroups of 256 threads (the fixed and the generic kernel), at most 128
    // workgroups that walk their tiles (the tiled kernel); every index inside the kernels is 64-bit.  HIP refuses a launch of 2^32 or
    // more threads in x, so the single batch is taken below 2^31 rows (2^31 + 255 threads at the most); a longer rollout goes row by
    // row, each row under pcc_policy_act_pop's own limits.
    if (n_members == 1 && row_step == 1 && (int64_t)T * n_envs <= (int64_t)0x7fffffff)
        return pcc_policy_act_pop(obs, (int64_t)T * n_envs, obs_dim, params, param_stride, 1, h1, h2, nullptr, mean_out, nullptr, nullptr,
                                  value_out, stream);
    for (int t = 0; t < T; t += row_step) {
        const int64_t at = (int64_t)t * n_envs;
        const int rc = pcc_policy_act_pop(obs + at * obs_dim, n_envs, obs_dim, params, param_stride, n_members, h1, h2, nullptr,
                                          mean_out ? mean_out + at : nullptr, nullptr, nullptr, value_out ? value_out + at : nullptr, stream);
        if (rc != 0) return rc;
        if (t > INT32_MAX - row_step) break;
    }
    return 0;
}
