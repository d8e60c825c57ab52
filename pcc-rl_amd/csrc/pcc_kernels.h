// pcc_kernels.h -- the launch functions of the kernel files (each .hip defines its kernels and the host function that
// launches them; pcc_sim.hip, the C ABI, calls these).  One translation unit per kernel family, so that every kernel
// is compiled -- and register-allocated -- on its own.
#pragma once
#include "pcc_dev.h"
#include "pcc_policy_dev.h"

#include <type_traits>

namespace pcc {

// What the launch functions are handed as one value each (the bundles end at the launch call: kernel parameters are spelled out)
struct StepOut { float *obs, *reward; uint8_t *done; double *steps; };   // where one step writes its rows (any of them NULL)
struct Actions { const void *p; int f64; };                              // the caller's action array, fp32 or fp64 (or none)
struct Warm { int on; uint32_t mi; int last; };   // a warm-up interval of a reset (ns:478-479): whether, which of the two, the last

// run-time (ns, flag) -> f(std::integral_constant<int, NS>, std::bool_constant<FLAG>): a generic lambda launches that instantiation
template <class F>
void dispatch_ns_flag(const int ns, const bool flag, F &&f) {
    if (ns == 1) { if (flag) f(std::integral_constant<int, 1>{}, std::true_type{}); else f(std::integral_constant<int, 1>{}, std::false_type{}); }
    else { if (flag) f(std::integral_constant<int, 2>{}, std::true_type{}); else f(std::integral_constant<int, 2>{}, std::false_type{}); }
}

// pcc_send.hip: both kinds of workgroup in one launch -- wave_wgs wave-path workgroups, then light_wgs light workgroups (with
// lists both are multiples of Dev::parts: workgroup b works for partition b % parts).
void launch_send(const Dev &d, bool trace, unsigned light_wgs, unsigned wave_wgs, unsigned light_front, hipStream_t st, int read_buf,
                 int zero_buf, const Warm &warm, int gate, const Actions &act);
// pcc_send_restart.hip.  grid: workgroups of 4 wavefronts, restart items dealt statically.
void launch_send_restart(const Dev &d, bool trace, unsigned grid, hipStream_t st, int read_buf, const Actions &act);
// ... refill_kernel: the shadows of the envs in refill row `row` (their next episodes: new links + warm-up intervals)
void launch_refill(const Dev &d, unsigned grid, hipStream_t st, uint32_t row, uint32_t fill_seq);
// pcc_retire.hip.  pol: the policy epilogue (pcc_rollout; one sender, not noise, not warm): every env's next action
void launch_retire(const Dev &d, bool noise, unsigned grid, hipStream_t st, int read_buf, int fill_buf, const Warm &warm, int gate,
                   int restart, const StepOut &out, const Actions &act, const PolicyArgs *pol = nullptr);
// pcc_noise_sorted.hip: a latency-noise interval run ahead of the retire launch (only_small: the first instance alone)
void launch_noise_sorted(const Dev &d, hipStream_t st, const Warm &warm, int gate, const Actions &act, int only_small);
// pcc_fused.hip: both halves of a full-size step in one launch (an env's retire half follows its own send half); grid =
// wave_wgs workgroups that start with the wave-path work + the rest, both multiples of Dev::parts
void launch_step_fused(const Dev &d, bool trace, unsigned grid, unsigned wave_wgs, unsigned light_front, hipStream_t st, int read_buf, int fill_buf, int zero_buf,
                       int retire_on, const Actions &act, const StepOut &out);
void launch_clear_list_buffer(const Dev &d, hipStream_t st, int buf);
int fused_resident_blocks(int ns, bool trace);   // workgroups of step_fused_kernel a compute unit holds at once (0: unknown)
// pcc_small.hip
// n_steps steps inside one launch: step t takes actions + t * act_stride bytes and writes row t of every output
// pol: the policy epilogue (pcc_rollout; one sender): step t reads its actions from pol's act rows (not `actions`), and every
// step but the last leaves the next step's action there
void launch_step_small(const Dev &d, bool trace, hipStream_t st, const Actions &act, const StepOut &out, int n_steps, int64_t act_stride,
                       const PolicyArgs *pol = nullptr);
void launch_reset_init(const Dev &d, hipStream_t st, const uint8_t *mask, int use_done, int gate, int all_envs, float *obs_out);
void launch_forget_ring_slots(const Dev &d, hipStream_t st);

constexpr int kRetireEnvsPerBlockNarrow = 16;  // envs of a retire workgroup at 8 lanes per env (16 lanes: half)

}  // namespace pcc
