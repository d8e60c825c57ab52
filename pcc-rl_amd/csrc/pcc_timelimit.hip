// pcc_timelimit.hip -- time-limit bootstrapping: the terminal observations of a rollout rebuilt from its own rows, and the advantage
// estimation that bootstraps from their values at a done (include/pcc_policy.h: pcc_terminal_obs, pcc_gae_boot, pcc_gae_boot_pop;
// DESIGN.md section 26).
//
//   terminal_obs_kernel  grid (ceil(n_envs / 256)), 256 threads: lane = env.  The lane walks its T done bytes in step order -- the
//                        loads are coalesced across the lanes, eight steps' loads are issued before they are looked at -- and counts
//                        its dones.  A row with a done in the wavefront (a ballot) is copied by the whole wavefront: the terminal row
//                        of env i after step t is obs[t][i][F .. H F) followed by (float)(steps[t][i][cols[f]] / scales[f]), into
//                        term_obs[slot][i], slot = the lane's count before this done.  Two ways to share the copy, picked per ballot
//                        by the number of wavefront passes each takes: the hits one after the other, passes of 64 lanes over the
//                        H F entries of one hit (few hits: envs out of lockstep); or the wavefront's 64 envs' rows as one contiguous
//                        run of 64 H F entries, H F passes whatever the number of hits, the lanes of envs without a hit idle (a burst:
//                        the batch in lockstep).  After the walk the slots an env did not reach are written as zeros, again over the
//                        contiguous run of the wavefront's rows of each slot.
//   gaeboot_kernel       gae_kernel of pcc_ppo.hip (thread = env, T steps backwards, blockIdx.y = member) with the same operations in
//                        the same order; at a done the next value is term_val[slot][i] -- slot counted down from term_count[i] -- and
//                        the running sum restarts at delta.
//
// Every element has one writer and no lane waits for another workgroup: no atomics, the same inputs give the same bits.  A unit of its
// own (see pcc_obsnorm.hip: adding kernels to an existing unit moves the old kernels' schedules).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pcc_policy.h"

namespace {

constexpr int kTlThreads = 256;
constexpr int kTlWave = 64;
constexpr int kTlUnroll = 8;        // steps whose done loads are in flight together
constexpr int kTlMaxFeatures = 16;  // the env's limit (csrc/pcc_retire_env.h: nf0, nf1)
constexpr int kTlStepCols = 19;     // a step record (include/pcc_sim.h: PCC_STEP_COLS)
constexpr int kTlMaxMembers = 1024;

struct TermFeatures {   // by value (entries past F: column 0, scale 1 -- never read)
    int32_t col[kTlMaxFeatures];
    double scale[kTlMaxFeatures];
};

// Entry x of the terminal row of one env: from its observation row before the step (obs_row) and the step's record (step_row).
// The new features are the retire epilogue's double division and its cast.  (col / scale are read with the lane's own index straight
// from the kernel's argument segment: loads, no copy of the arrays into registers or scratch.)
__device__ __forceinline__ float terminal_entry(const float *__restrict__ obs_row, const double *__restrict__ step_row, int x, int keep,
                                                int F, const TermFeatures &P) {
    if (x < keep) return obs_row[x + F];
    return (float)(step_row[P.col[x - keep]] / P.scale[x - keep]);
}

__global__ __launch_bounds__(kTlThreads) void terminal_obs_kernel(const float *__restrict__ obs, const double *__restrict__ steps,
                                                                  const uint8_t *__restrict__ done, int T, int64_t n_envs, int HF, int F,
                                                                  TermFeatures P, int n_slots, float *__restrict__ term_obs,
                                                                  int32_t *__restrict__ term_count) {
    const int lane = threadIdx.x & (kTlWave - 1);
    const int64_t i = (int64_t)blockIdx.x * kTlThreads + threadIdx.x;   // the env
    const int64_t i0 = i - lane;                                        // the wavefront's first env
    const bool live = i < n_envs;
    const int keep = HF - F;
    const int run = kTlWave * HF;                  // entries of the wavefront's 64 rows of one [n_envs][HF] block
    const int hit_passes = (HF + kTlWave - 1) / kTlWave;
    const int de = kTlWave / HF, dx = kTlWave - de * HF;   // position p + 64 of a run is entry x + dx of env e + de, or one env on
    const uint8_t *dp = done + (live ? i : 0);
    int cnt = 0;

    // one row t: d = this lane's done byte (0 for a lane past the batch)
    auto row = [&](int t, uint8_t d) {
        const bool hit = d != 0;
        const unsigned long long hits = __ballot(hit);
        if (hits == 0ull) return;   // (wave-uniform)
        const float *obs_t = obs + (int64_t)t * n_envs * HF;
        const double *steps_t = steps + (int64_t)t * n_envs * kTlStepCols;
        if (__popcll(hits) * hit_passes < HF) {
            // few hits: one after the other, the wavefront over the entries of the hit's row
            unsigned long long rest = hits;
            while (rest) {
                const int e = __ffsll((long long)rest) - 1;
                rest &= rest - 1;
                const int slot = __shfl(cnt, e);
                if (slot >= n_slots) continue;   // counted, not stored
                const int64_t env = i0 + e;
                float *dst = term_obs + ((int64_t)slot * n_envs + env) * HF;
                for (int x = lane; x < HF; x += kTlWave)
                    dst[x] = terminal_entry(obs_t + env * HF, steps_t + env * kTlStepCols, x, keep, F, P);
            }
        } else {
            // a burst: the 64 rows as one run, lane after lane; (e, x) = the env and the entry of position p, kept without a division
            int e = lane / HF, x = lane - e * HF;
            for (int p = lane; p < run; p += kTlWave) {
                const int slot = __shfl(cnt, e);
                if (((hits >> e) & 1ull) && slot < n_slots) {
                    const int64_t env = i0 + e;
                    term_obs[((int64_t)slot * n_envs + env) * HF + x] =
                        terminal_entry(obs_t + env * HF, steps_t + env * kTlStepCols, x, keep, F, P);
                }
                e += de;
                x += dx;
                if (x >= HF) {
                    x -= HF;
                    e++;
                }
            }
        }
        if (hit) cnt++;
    };

    int t = 0;
    for (; t + kTlUnroll <= T; t += kTlUnroll) {
        uint32_t bits = 0;   // bit u: a done in row t + u
#pragma unroll
        for (int u = 0; u < kTlUnroll; u++) bits |= (live && dp[(int64_t)(t + u) * n_envs] != 0 ? 1u : 0u) << u;
        if (__ballot(bits != 0) == 0ull) continue;   // (wave-uniform: no done in these rows, the usual case)
#pragma unroll 1
        for (int u = 0; u < kTlUnroll; u++) row(t + u, (uint8_t)((bits >> u) & 1u));
    }
#pragma unroll 1
    for (; t < T; t++) row(t, live ? dp[(int64_t)t * n_envs] : (uint8_t)0);

    if (live) term_count[i] = cnt;

    // the slots this env did not reach: zeros (every row handed to the policy kernels is finite)
    for (int k = 0; k < n_slots; k++) {
        const unsigned long long empty = __ballot(live && cnt <= k);
        if (empty == 0ull) continue;
        float *dst = term_obs + ((int64_t)k * n_envs + i0) * HF;
        int e = lane / HF, x = lane - e * HF;
        for (int p = lane; p < run; p += kTlWave) {
            if ((empty >> e) & 1ull) dst[p] = 0.0f;
            e += de;
            x += dx;
            if (x >= HF) {
                x -= HF;
                e++;
            }
        }
    }
}

// gae_kernel (pcc_ppo.hip) with the bootstrap at a done.  c counts the env's dones in the rows below the one being looked at.
__global__ void gaeboot_kernel(const float *__restrict__ rew, const float *__restrict__ val, const uint8_t *__restrict__ done,
                                const float *__restrict__ last_val, const float *__restrict__ term_val,
                                const int32_t *__restrict__ term_count, int n_slots, int T, int64_t n, int64_t n_member,
                                const float *__restrict__ hyper, float gamma_arg, float lam_arg, float *__restrict__ adv,
                                float *__restrict__ ret) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_member) return;
    const int64_t i = (int64_t)blockIdx.y * n_member + r;
    const float gamma = hyper ? hyper[blockIdx.y * 8 + 3] : gamma_arg, lam = hyper ? hyper[blockIdx.y * 8 + 4] : lam_arg;
    float next_v = last_val[i], run = 0.0f;
    int c = term_count[i];
    for (int t = T - 1; t >= 0; t--) {
        const int64_t k = (int64_t)t * n + i;
        const float v = val[k];
        if (done[k]) {
            c--;   // this done's slot: the dones before it
            const float v_term = (c >= 0 && c < n_slots) ? term_val[(int64_t)c * n + i] : 0.0f;
            const float delta = rew[k] + gamma * v_term - v;
            run = delta;
        } else {
            const float alive = 1.0f;
            const float delta = rew[k] + gamma * next_v * alive - v;
            run = delta + gamma * lam * alive * run;
        }
        adv[k] = run;
        ret[k] = run + v;
        next_v = v;
    }
}

int launch_gae_boot(const float *rewards, const float *values, const uint8_t *dones, const float *last_value, const float *term_value,
                    const int32_t *term_count, int n_slots, int T, int64_t n_envs, int n_members, const float *hyper, float gamma,
                    float lam, float *adv_out, float *ret_out, void *stream) {
    // (every refusal comes before any HIP call: a host without a device gives the same answers)
    if (!rewards || !values || !dones || !last_value || !term_value || !term_count || !adv_out || !ret_out) return -1;
    if (T < 1 || n_envs < 1 || n_slots < 1) return -1;
    if (n_members < 1 || n_members > kTlMaxMembers || n_envs % n_members != 0) return -1;
    const int64_t n_member = n_envs / n_members;
    if ((n_member + 255) / 256 > 0x7fffffff) return -1;
    hipLaunchKernelGGL(gaeboot_kernel, dim3((unsigned)((n_member + 255) / 256), (unsigned)n_members), dim3(256), 0,
                       static_cast<hipStream_t>(stream), rewards, values, dones, last_value, term_value, term_count, n_slots, T, n_envs,
                       n_member, hyper, gamma, lam, adv_out, ret_out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace

extern "C" int pcc_terminal_obs(const float *obs, const double *steps, const uint8_t *done, int T, int64_t n_envs, int H, int F,
                                const int32_t *cols, const double *scales, int n_slots, float *term_obs_out, int32_t *term_count_out,
                                void *stream) {
    if (!obs || !steps || !done || !cols || !scales || !term_obs_out || !term_count_out) return -1;
    if (T < 1 || n_envs < 1 || n_slots < 1 || H < 1 || F < 1 || F > kTlMaxFeatures) return -1;
    if (H > 0x7fffffff / (kTlWave * F)) return -1;   // (the wavefront's run of 64 rows is indexed in 32 bits)
    TermFeatures P;
    for (int f = 0; f < kTlMaxFeatures; f++) {
        P.col[f] = 0;
        P.scale[f] = 1.0;
    }
    for (int f = 0; f < F; f++) {
        if (cols[f] < 0 || cols[f] >= kTlStepCols || !std::isfinite(scales[f]) || !(scales[f] > 0.0)) return -1;
        P.col[f] = cols[f];
        P.scale[f] = scales[f];
    }
    const int64_t blocks = (n_envs + kTlThreads - 1) / kTlThreads;
    if (blocks > 0x7fffffff) return -1;
    hipLaunchKernelGGL(terminal_obs_kernel, dim3((unsigned)blocks), dim3(kTlThreads), 0, static_cast<hipStream_t>(stream), obs, steps,
                       done, T, n_envs, H * F, F, P, n_slots, term_obs_out, term_count_out);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int pcc_gae_boot(const float *rewards, const float *values, const uint8_t *dones, const float *last_value,
                            const float *term_value, const int32_t *term_count, int n_slots, int T, int64_t n_envs, float gamma,
                            float lam, float *adv_out, float *ret_out, void *stream) {
    return launch_gae_boot(rewards, values, dones, last_value, term_value, term_count, n_slots, T, n_envs, 1, nullptr, gamma, lam,
                           adv_out, ret_out, stream);
}

extern "C" int pcc_gae_boot_pop(const float *rewards, const float *values, const uint8_t *dones, const float *last_value,
                                const float *term_value, const int32_t *term_count, int n_slots, int T, int64_t n_envs, int n_members,
                                const float *hyper, float *adv_out, float *ret_out, void *stream) {
    if (!hyper) return -1;
    return launch_gae_boot(rewards, values, dones, last_value, term_value, term_count, n_slots, T, n_envs, n_members, hyper, 0.0f,
                           0.0f, adv_out, ret_out, stream);
}
