/*
 * pcc_policy.h -- C ABI of the fused policy forward of the on-device PPO caller (libpcc_sim.so).
 *
 * Not part of the reference's env path: the reference's agent is stable-baselines PPO1 on
 * TensorFlow 1 (src/gym/stable_solve.py:39-58), a caller of the env.  This entry point evaluates that
 * script's policy architecture (ibid. :39-45: pi and vf MLPs with two tanh hidden layers, --arch, and a
 * state-independent log-std) for a whole env batch in one kernel launch, so that the batched env
 * (pcc_sim.h) is not starved by the agent.  fp32.
 */
#ifndef PCC_POLICY_H
#define PCC_POLICY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * obs       [n_envs][obs_dim] float32, device (the observation rows pcc_step / pcc_reset wrote)
 * params    device floats: pi {W1[h1][obs_dim], b1[h1], W2[h2][h1], b2[h2], W3[h2], b3, log_std},
 *           then vf {the same without log_std} -- row-major like torch.nn.Linear.weight
 * noise     [n_envs] standard-normal draws, device; NULL = deterministic (act = mean, logp of the mean)
 * mean_out, act_out, logp_out, value_out   [n_envs] each, device; any may be NULL
 * stream    HIP stream; nothing synchronizes
 * Returns 0 for every shape of the domain of pcc_ppo_supported (1 <= obs_dim <= 128, 1 <= h1, h2 <= 64: obs_dim, h1 and h2
 * are run-time values; --arch 32,16 at 3, 6, 12, 30, 36 or 60 observations runs a fully unrolled kernel -- the table
 * PCC_FIXED_OBS_LENGTHS of csrc/pcc_policy_dev.h, where PolicyLayout states the layout of `params` for every kernel); -1 bad arguments
 * (NULL obs / params, n_envs < 1, a hidden size outside 1 .. 64); -2 obs_dim outside 1 .. 128 (the caller falls back to its
 * framework path); -3 launch failure.
 */
int pcc_policy_act(const float *obs, int64_t n_envs, int obs_dim, const float *params, int h1, int h2,
                   const float *noise, float *mean_out, float *act_out, float *logp_out, float *value_out,
                   void *stream);

/*
 * One optimiser step of PPO1's objective on one minibatch of a rollout -- what stable-baselines does per minibatch
 * inside PPO1.learn (src/gym/stable_solve.py:52: clip 0.2, entropy coefficient, Adam; its policy :39-45) -- as two
 * launches: the gradient of  -mean(min(r A, clip(r, 1 - clip, 1 + clip) A)) + 0.5 mean((v - ret)^2) - ent_coef * entropy
 * over the samples perm[start .. start + count) (perm NULL: start .. start + count), then Adam (torch.optim.Adam's
 * arithmetic) on `params` in place.  All pointers are device memory, fp32 (perm: int64).
 *
 * obs [n][obs_dim], act / logp_old / adv / ret [n]   the flattened rollout (adv already normalised by the caller)
 * params    the block pcc_policy_act reads; adam_m / adam_v [n_params] the optimiser state; adam_step = 1, 2, ...
 * lr == 0   gradient only: nothing is updated (adam_m / adam_v may be NULL)
 * scratch   pcc_ppo_scratch_floats(obs_dim, h1, h2) floats
 * grad_out  [n_params] or NULL: the gradient that was applied
 * stats_out [4] or NULL: {mean clipped surrogate (= -policy loss), mean squared value error (= 2 x value loss),
 *           fraction of samples with |r - 1| > clip, 0}
 * Returns 0; -1 bad arguments; -2 no kernel for this shape: one outside the domain of pcc_ppo_supported (the caller falls
 * back to its framework path); -3 launch failure.
 *
 * pcc_ppo_supported: 1 if both pcc_policy_act and pcc_ppo_minibatch_step have a kernel for a policy of two tanh hidden layers
 * h1, h2 on obs_dim observations (1 <= obs_dim <= 128, 1 <= h1, h2 <= 64), else 0.  Host only: needs no GPU.
 */
int pcc_ppo_supported(int obs_dim, int h1, int h2);
int pcc_ppo_scratch_floats(int obs_dim, int h1, int h2);
int pcc_ppo_minibatch_step(const float *obs, const float *act, const float *logp_old, const float *adv, const float *ret,
                           const int64_t *perm, int64_t start, int64_t count, int obs_dim, int h1, int h2, float *params,
                           float *adam_m, float *adam_v, int adam_step, float lr, float beta1, float beta2, float eps,
                           float clip, float ent_coef, float *scratch, float *grad_out, float *stats_out, void *stream);

/*
 * Generalised advantage estimation over the [T][n_envs] rows of a rollout, one launch: dones[t][i] != 0 marks that env i
 * was reset after step t.  adv_out / ret_out [T][n_envs].
 */
int pcc_gae(const float *rewards, const float *values, const uint8_t *dones, const float *last_value, int T, int64_t n_envs,
            float gamma, float lam, float *adv_out, float *ret_out, void *stream);

/*
 * A population: n_members independent policies on n_members equal slices of one env batch.  Member m owns the envs (the
 * columns of [T][n_envs] rows) [m * n_envs / n_members, (m + 1) * n_envs / n_members); n_envs % n_members != 0 returns -1;
 * 1 <= n_members <= 1024.  Parameter blocks (params, adam_m, adam_v, grad_out) are [n_members][param_stride] floats: each row
 * has the layout `params` has above in its first n_params floats; param_stride >= n_params and a multiple of 64 floats (every
 * member's block 256-byte aligned), anything else returns -1; the padding is never read or written.
 * hyper     caller-owned device floats [n_members][8]: {lr, clip, ent_coef, gamma, lam, max_grad_norm, 0, 0}; column 5 is read
 *           by pcc_ppo_minibatch_step_clip_pop alone (below), every other entry point carries it along unread
 *
 * pcc_policy_act_pop: pcc_policy_act for every member in ONE launch (the member is a grid dimension).  Every output is
 * bit-identical to n_members calls of pcc_policy_act on the members' row slices with params + m * param_stride: a member's
 * slice is cut into workgroups and tiles exactly as a stand-alone launch over its rows (no divisibility is asked of the member
 * size), and in the --arch 32,16 kernel a member's weights stay wave-uniform scalar loads.  The domain and the return codes of
 * pcc_policy_act.
 *
 * pcc_ppo_minibatch_step_pop: pcc_ppo_minibatch_step for every member in TWO launches (gradient, Adam; the member is a grid
 * dimension).  perm is required: member m takes the samples perm[m * perm_stride + start .. + count), indices into the SAME
 * flattened [T * N] rollout arrays for every member.  Each member's grid and order of partial sums are those of a stand-alone
 * call with the same count, so params, adam_m, adam_v, grad_out ([n_members][param_stride], or NULL) and stats_out
 * ([n_members][4], or NULL) are bit-identical to n_members calls of pcc_ppo_minibatch_step with perm + m * perm_stride and
 * that member's lr, clip and ent_coef.  A member with lr == 0 in hyper is gradient-only, as there.  scratch is n_members x
 * pcc_ppo_scratch_floats(obs_dim, h1, h2) floats.  adam_step >= 1 and adam_m / adam_v non-NULL always: the host cannot see
 * the learning rates.  Returns as pcc_ppo_minibatch_step.
 *
 * pcc_gae_pop: pcc_gae with gamma and lambda read per member from hyper; bit-identical to pcc_gae on a contiguous copy of a
 * member's columns.
 */
int pcc_policy_act_pop(const float *obs, int64_t n_envs, int obs_dim, const float *params, int64_t param_stride,
                       int n_members, int h1, int h2, const float *noise, float *mean_out, float *act_out,
                       float *logp_out, float *value_out, void *stream);
int pcc_ppo_minibatch_step_pop(const float *obs, const float *act, const float *logp_old, const float *adv, const float *ret,
                       const int64_t *perm, int64_t perm_stride, int64_t start, int64_t count, int obs_dim, int h1, int h2,
                       float *params, float *adam_m, float *adam_v, int64_t param_stride, int n_members, const float *hyper,
                       int adam_step, float beta1, float beta2, float eps, float *scratch, float *grad_out, float *stats_out,
                       void *stream);
int pcc_gae_pop(const float *rewards, const float *values, const uint8_t *dones, const float *last_value, int T,
                int64_t n_envs, int n_members, const float *hyper, float *adv_out, float *ret_out, void *stream);

/*
 * The step between two generations of a population (population-based training, Jaderberg et al. 2017: truncation selection,
 * copy, perturb) on the blocks above, ONE launch, no copy to the host, nothing synchronizes.  Arch-agnostic: it takes n_params.
 * score     [n_members] float64, larger is better
 * explore   [8][4] floats, one row per column of hyper: {factor_lo, factor_hi, min, max}
 * parent_out, rank_out   [n_members] int32; either may be NULL
 * Ordering: member a is better than b (a != b) when exactly one of the two scores is NaN and a's is not; else when neither is
 * NaN, score[a] != score[b] and score[a] > score[b]; else when a < b.  rank[m] = the number of members better than m: a
 * permutation of 0 .. n_members - 1, ties and +-0 broken by index, NaN last.
 * With n_valid the number of non-NaN scores and n_src = min(n_cut, n_valid), member m is replaced iff n_src > 0 and
 * rank[m] >= n_members - n_cut.  Its source: w = philox4x32_10(counter (m, generation, 0, 0), key (seed & 0xffffffff, seed >> 32)),
 * j = ((uint64)w[0] * n_src) >> 32, p = the member of rank j.  Sources have rank < n_src <= n_cut <= n_members / 2: no row is
 * both read and written.  The floats [0, n_params) of row p of params, adam_m and adam_v are copied to row m (the padding is
 * never read or written); hyper[m][c] = fminf(fmaxf(hyper[p][c] * f, explore[c][2]), explore[c][3]) for every column c, one
 * float32 multiply, f = explore[c][1] if bit c of w[1] is set, else explore[c][0] -- a row {1, 1, -inf, +inf} inherits the
 * value exactly; parent_out[m] = p.  Of a member that is not replaced nothing is written, and parent_out[m] = m.
 * rank_out[m] = rank[m] for every m.  The same arguments on the same inputs give the same bits.
 * Returns 0; -1, with nothing written and before any device call, for n_members outside 1 .. 1024, n_cut < 0 or 2 n_cut >
 * n_members, param_stride not a multiple of 64, n_params < 1 or > param_stride, a NULL score / params / adam_m / adam_v /
 * hyper / explore; -3 launch failure.
 */
int pcc_pbt_evolve(const double *score, int n_members, int n_cut, float *params, float *adam_m, float *adam_v,
                   int64_t param_stride, int64_t n_params, float *hyper, const float *explore, uint64_t seed,
                   uint32_t generation, int32_t *parent_out, int32_t *rank_out, void *stream);

/*
 * Observation normalisation: running per-member, per-feature moments of the raw observation rows, and
 * the standardised, clipped rows the policy kernels read.  All buffers are caller-owned device memory; everything is enqueued
 * on `stream`, nothing synchronizes.  Member m owns the columns [m * n_envs / n_members, (m + 1) * n_envs / n_members) of every
 * [.][n_envs][obs_dim] row block, as above.
 * stats     float64 [n_members][stat_stride], stat_stride >= 1 + 2 * obs_dim: row m is {count, mean[obs_dim], m2[obs_dim]}, m2 the
 *           sum of squared deviations; the padding is never read or written; all zeros is the empty state
 * norm      float32 [n_members][2 * obs_dim]: row m is {shift[obs_dim], scale[obs_dim]}
 *
 * pcc_obs_stats_update_pop, two launches: for every member the moments (n_b = T * n_envs / n_members, mean_b, m2_b) of its rows of
 * obs[T][n_envs][obs_dim], accumulated in float64 (partial moments per workgroup into scratch, then one workgroup per member
 * combines them in a fixed order), merged into row m of stats by Chan's formula -- n = n_a + n_b, d = mean_b - mean_a,
 * mean = mean_a + d * n_b / n, m2 = m2_a + m2_b + d * d * n_a * n_b / n; a row with count == 0 becomes the batch's moments -- and,
 * if norm != NULL, shift[d] = (float)mean[d], scale[d] = (float)(1.0 / sqrt(m2[d] / count + eps)): IEEE float64 arithmetic,
 * rounded to float32 once.  scratch is pcc_obs_stats_scratch_doubles(T, n_envs, obs_dim, n_members) doubles (host only; -1
 * outside the domain).
 *
 * pcc_obs_normalise_pop, one launch, one [n_envs][obs_dim] row block: out = fminf(fmaxf((x - shift[d]) * scale[d], -clip), clip),
 * three float32 operations, no contraction.  out == obs is allowed.
 *
 * No atomics, no hand-off between workgroups: the same inputs give the same bits, and a member's stats, norm and out are
 * bit-identical to the stand-alone call on a contiguous copy of its columns (a member is cut into workgroups exactly as a launch
 * over the member alone; no divisibility is asked of the member size).  pcc_obs_stats_update / pcc_obs_normalise are the
 * stand-alone forms: the same kernels with one member and stat_stride = 1 + 2 * obs_dim.
 * Returns 0; -1, with nothing written and before any device call, outside 1 <= obs_dim <= 128, 1 <= n_members <= 1024,
 * n_envs % n_members == 0, T >= 1, clip > 0, eps >= 0, stat_stride >= 1 + 2 * obs_dim, or for a NULL obs / stats / scratch / out
 * (pcc_obs_normalise_pop: a NULL norm too); -3 launch failure.
 */
int pcc_obs_stats_scratch_doubles(int T, int64_t n_envs, int obs_dim, int n_members);
int pcc_obs_stats_update_pop(const float *obs, int T, int64_t n_envs, int obs_dim, int n_members, double *stats,
                             int64_t stat_stride, float *norm, double eps, double *scratch, void *stream);
int pcc_obs_normalise_pop(const float *obs, int64_t n_envs, int obs_dim, int n_members, const float *norm, float clip,
                          float *out, void *stream);
int pcc_obs_stats_update(const float *obs, int T, int64_t n_envs, int obs_dim, double *stats, float *norm, double eps,
                         double *scratch, void *stream);
int pcc_obs_normalise(const float *obs, int64_t n_envs, int obs_dim, const float *norm, float clip, float *out, void *stream);

/*
 * The episode ledger: what every episode returned -- per env the running episode and the last finished
 * one, per member the totals of the finished episodes -- from the [T][n_envs] rows a rollout already holds.  One sender.  All
 * buffers are caller-owned device memory; everything is enqueued on `stream`, nothing synchronizes.  Member m owns the columns
 * [m * n_envs / n_members, (m + 1) * n_envs / n_members), as above.
 * reward    [T][n_envs] float32; done [T][n_envs] uint8, != 0: env i's episode ended with step t
 * steps     pcc_step_many's steps_out, [T][n_envs][PCC_STEP_COLS] float64 (include/pcc_sim.h), or NULL with n_channels == 1
 * cols      HOST array of n_channels - 1 column indices in [0, PCC_STEP_COLS); it is read before the call returns
 * Channels: C = n_channels, 1 <= C <= 8.  Channel 0 is (double)reward[t][i]; channel c >= 1 is steps[t][i][cols[c - 1]].  Finite
 * rewards and columns are the contract: a NaN or an infinity is summed like any other value and spoils the episode it belongs
 * to and the totals that episode enters (min / max then follow fmin / fmax), nothing else.
 * carry     float64 [n_envs][C], carry_len int32 [n_envs]: every env's running episode; all zeros is the empty state
 * last      float64 [n_envs][C], last_len int32 [n_envs]: every env's last finished episode; either may be NULL
 * totals    float64 [n_members][totals_stride], totals_stride >= 2 + 4 C: row m is {episodes, steps, then per channel sum, sumsq,
 *           min, max} of the channel totals of the member's finished episodes since the row was last zeroed.  All zeros is the
 *           empty state: with episodes == 0 on entry the min / max slots are not read.  Of a member without a finished episode
 *           in this call nothing in its row is written; the padding is never read or written.
 * scratch   pcc_episode_scratch_doubles(n_envs, n_members, n_channels) doubles (host only; -1 outside the domain)
 *
 * pcc_episode_update_pop, two launches.  For every env i, for t = 0 .. T - 1 in this order: carry[i][c] += x_c, one float64
 * addition per channel; carry_len[i] += 1; if done[t][i] != 0 the episode is finished: carry[i] / carry_len[i] go to last[i] /
 * last_len[i] and into the member's row -- episodes += 1, steps += carry_len[i], per channel with v = carry[i][c]: sum += v,
 * sumsq += v * v (no contraction), min, max -- and carry[i][:] = 0, carry_len[i] = 0.  So carry, carry_len, last and last_len
 * are specified bit for bit, a call over [0, T) and two calls over [0, T1) and [T1, T) leave the same bits in the four, and
 * with the column PCC_COL_REWARD as a channel, last reproduces the env's own last_return bit for bit.  episodes, steps, min and
 * max are exact.  sum and sumsq add a member's episodes in a fixed order that is the implementation's: lane = env sums its own
 * episodes in step order, a workgroup of 256 lanes its lanes in a fixed tree, one workgroup per member the workgroups' partials
 * in index order, and the result is added to the row.
 *
 * No atomics, no hand-off between workgroups: the same inputs give the same bits, and a member's row, carry and last are
 * bit-identical to the stand-alone call on a contiguous copy of its columns (a member is cut into workgroups exactly as a launch
 * over the member alone; no divisibility is asked of the member size).  pcc_episode_update is the stand-alone form: the same
 * kernels with one member.
 * Returns 0; -1, with nothing written and before any device call, outside 1 <= n_channels <= 8, T >= 1, 1 <= n_members <= 1024,
 * n_envs >= 1, n_envs % n_members == 0, totals_stride >= 2 + 4 n_channels, for a NULL reward / done / carry / carry_len / totals /
 * scratch, a NULL steps or cols with n_channels > 1, or a column index out of range; -3 launch failure.
 */
int pcc_episode_scratch_doubles(int64_t n_envs, int n_members, int n_channels);
int pcc_episode_update_pop(const float *reward, const uint8_t *done, const double *steps, const int32_t *cols, int n_channels,
                           int T, int64_t n_envs, int n_members, double *carry, int32_t *carry_len, double *last,
                           int32_t *last_len, double *totals, int64_t totals_stride, double *scratch, void *stream);
int pcc_episode_update(const float *reward, const uint8_t *done, const double *steps, const int32_t *cols, int n_channels, int T,
                       int64_t n_envs, double *carry, int32_t *carry_len, double *last, int32_t *last_len, double *totals,
                       int64_t totals_stride, double *scratch, void *stream);

/*
 * Reward normalisation: the running per-member variance of every env's discounted return, and the reward
 * rows divided by its square root and clipped -- the norm_reward half of stable-baselines' VecNormalize, from the [T][n_envs] rows a
 * rollout already holds.  One sender.  All buffers are caller-owned device memory; everything is enqueued on `stream`, nothing
 * synchronizes.  Member m owns the columns [m * n_envs / n_members, (m + 1) * n_envs / n_members), as above.
 * reward    [T][n_envs] float32; done [T][n_envs] uint8, != 0: env i's episode ended with step t
 * hyper     the population's [n_members][8] float32 block: column 3 is the member's gamma, as pcc_gae_pop reads it
 * ret_carry float64 [n_envs]: every env's running discounted return; all zeros is the empty state
 * stats     float64 [n_members][stat_stride], stat_stride >= 3: row m is {count, mean, m2} of the member's samples, m2 the sum of
 *           squared deviations; the padding is never read or written; all zeros is the empty state
 * scale     float32 [n_members], or NULL
 * scratch   pcc_return_scratch_doubles(T, n_envs, n_members) doubles (host only; -1 outside the domain)
 *
 * pcc_return_stats_update_pop, two launches.  For every env i of member m, with R = ret_carry[i], for t = 0 .. T - 1 in this order:
 * R = R * (double)gamma_m + (double)reward[t][i], one float64 multiplication and one float64 addition, no contraction; this R is
 * one sample of member m's batch; then, if done[t][i] != 0, R = 0 (VecNormalize's order: the sample is taken before the reset).
 * R goes back to ret_carry[i].  So ret_carry is specified bit for bit, and a call over [0, T) and two calls over [0, T1) and
 * [T1, T) leave the same bits in it.  The batch's moments (n_b = T * n_envs / n_members, mean_b, m2_b) are accumulated in float64 in
 * a fixed order that is the implementation's: lane = env reduces its own T samples in step order, a workgroup of 256 lanes its
 * lanes in a fixed tree, one workgroup per member the workgroups' partials in index order.  They are merged into row m of stats by
 * Chan's formula as stated for the observation moments above -- a row with count == 0 becomes the batch's moments; count is exact
 * -- and, if scale != NULL, scale[m] = (float)(1.0 / sqrt(m2 / count + eps)): IEEE float64 arithmetic, rounded to float32 once.
 * Finite rewards are the contract: a NaN or an infinity is carried like any other value and spoils the env's running return
 * until its next done, and the member's moments.
 *
 * pcc_reward_normalise_pop, one launch over the [T][n_envs] rows: out = fminf(fmaxf(r * scale[m], -clip), clip), m the member that
 * owns the column: two float32 operations, no mean shift (as VecNormalize).  out == reward is allowed.
 *
 * No atomics, no hand-off between workgroups: the same inputs give the same bits, and a member's row, scale, ret_carry and out are
 * bit-identical to the stand-alone call on a contiguous copy of its columns (a member is cut into workgroups exactly as a launch
 * over the member alone; no divisibility is asked of the member size).  pcc_return_stats_update / pcc_reward_normalise are the
 * stand-alone forms: the same kernels with one member, stat_stride = 3, gamma as an argument and scale[1].
 * Returns 0; -1, with nothing written and before any device call, outside T >= 1, n_envs >= 1, 1 <= n_members <= 1024,
 * n_envs % n_members == 0, stat_stride >= 3, eps >= 0, clip > 0, or for a NULL reward / done / hyper / ret_carry / stats / scratch /
 * out (pcc_reward_normalise_pop: a NULL scale too); -3 launch failure.
 */
int pcc_return_scratch_doubles(int T, int64_t n_envs, int n_members);
int pcc_return_stats_update_pop(const float *reward, const uint8_t *done, int T, int64_t n_envs, int n_members,
                                const float *hyper, double *ret_carry, double *stats, int64_t stat_stride, float *scale,
                                double eps, double *scratch, void *stream);
int pcc_reward_normalise_pop(const float *reward, int T, int64_t n_envs, int n_members, const float *scale, float clip,
                             float *out, void *stream);
int pcc_return_stats_update(const float *reward, const uint8_t *done, int T, int64_t n_envs, float gamma, double *ret_carry,
                            double *stats, float *scale, double eps, double *scratch, void *stream);
int pcc_reward_normalise(const float *reward, int T, int64_t n_envs, const float *scale, float clip, float *out, void *stream);

/*
 * Update diagnostics and the KL guard: what an update did to the policy -- per member the approximate KL
 * divergence between the rollout's policy and the updated one, the clip fraction over the whole rollout, the explained variance of
 * the value function -- from the [T][n_envs] rows a rollout already holds, and the per-member decision to stop updating, taken on the
 * device.  One sender.  All buffers are caller-owned device memory; everything is enqueued on `stream`, nothing synchronizes.
 * Member m owns the columns [m * n_envs / n_members, (m + 1) * n_envs / n_members), as above.
 *
 * pcc_policy_act_rows_pop: the deterministic forward (noise == NULL) of pcc_policy_act_pop on the rows t = 0, row_step, 2 row_step,
 * ... < T of obs[T][n_envs][obs_dim], into the same rows of mean_out / value_out [T][n_envs]; either may be NULL; no other row is
 * written.  One library call; inside it the launches are pcc_policy_act_pop's -- one per row, or, with one member and row_step == 1,
 * one over the T * n_envs rows as a single batch -- and every output is bit-identical to calling pcc_policy_act_pop row by row.
 * The domain and the return codes of pcc_policy_act_pop, plus -1 for T < 1 or row_step < 1;
 * every -1 comes before any device call.
 *
 * pcc_update_diag_pop, two launches, over the rows t = 0, row_step, ... < T (the selected rows):
 * act, logp_old, mean_new, ret, val   [T][n_envs] float32: the rollout's actions and log-probabilities, the UPDATED policy's means
 *           (pcc_policy_act_rows_pop), the returns the value function was fitted to and the rollout's values
 * params, param_stride   the population's parameter blocks; log_std = params[m * param_stride + log_std_index]
 * hyper     the population's [n_members][8] float32 block: column 1 is the member's clip range
 * diag      float64 [n_members][diag_stride], diag_stride >= 8: row m is {count, approx_kl, clip_fraction, explained_variance,
 *           max_abs_log_ratio, var_ret, var_resid, nonfinite}; the padding is never read or written
 * stop      int32 [n_members], sticky: 0, or the epoch at which the member was stopped; the caller zeroes it at the start of an
 *           update.  hyper_live: float32 [n_members][8].  The two may be NULL only together: diagnostics alone
 * scratch   pcc_update_diag_scratch_doubles(T, row_step, n_envs, n_members) doubles (host only; -1 outside the domain)
 * Per sample of a selected row, in float32 without contraction: inv = expf(-log_std) (libm's), z = (act - mean_new) * inv,
 * lp = -0.5f * z * z - log_std - log(2 pi) / 2 (the Gaussian head's log-probability), d32 = lp - logp_old.  Then in float64:
 * d = (double)d32, k = expm1(d) - d; the sample counts as clipped iff fabs(expm1(d)) > (double)hyper[m][1]; e = (double)ret -
 * (double)val.  approx_kl = the mean of k; clip_fraction = clipped / count; var_ret and var_resid the population variances (m2 /
 * count) of ret and of e, accumulated as {n, mean, m2} with Chan's merge as stated for the observation moments above;
 * explained_variance = 1 - var_resid / var_ret, NaN when var_ret == 0; max_abs_log_ratio = the maximum of fabs(d) by fmax from 0 (a
 * NaN sample does not enter it); nonfinite = the number of samples whose d is not finite.  count, the clipped count and nonfinite
 * are exact.  The float64 sums are added in a fixed order that is the implementation's: lane = env adds its own rows in step order,
 * a wavefront its lanes in a fixed tree, a workgroup of 256 lanes its four wavefronts in index order, one workgroup per member the
 * workgroups' partials in index order.
 * The decision, per member, after its row is written, if stop != NULL: if stop[m] == 0 && kl_limit > 0 && !(approx_kl <= kl_limit)
 * then stop[m] = epoch -- a NaN approx_kl stops the member; kl_limit <= 0 never stops.  Then hyper_live[m][0 .. 8) = hyper[m][0 .. 8)
 * and hyper_live[m][0] = 0.0f iff stop[m] != 0: pcc_ppo_minibatch_step_pop with hyper_live in place of hyper treats a stopped member
 * as gradient-only and leaves its parameters and moments alone.
 *
 * No atomics, no hand-off between workgroups: the same inputs give the same bits, and a member's row is bit-identical to the
 * stand-alone call on a contiguous copy of its columns (a member is cut into workgroups exactly as a launch over the member alone; no
 * divisibility is asked of the member size).  pcc_update_diag is the stand-alone form: the same kernels with one member, diag [8],
 * the clip range as an argument, log_std = params[log_std_index], no decision.
 * Returns 0; -1, with nothing written and before any device call, for T < 1, row_step < 1, n_envs < 1, n_members outside 1 .. 1024,
 * n_envs % n_members != 0, diag_stride < 8, epoch < 1, log_std_index outside [0, param_stride), param_stride not a multiple of 64,
 * a NULL act / logp_old / mean_new / ret / val / params / hyper / diag / scratch, or exactly one of stop and hyper_live NULL; -3
 * launch failure.
 */
int pcc_policy_act_rows_pop(const float *obs, int T, int row_step, int64_t n_envs, int obs_dim, const float *params,
                            int64_t param_stride, int n_members, int h1, int h2, float *mean_out, float *value_out, void *stream);
int pcc_update_diag_scratch_doubles(int T, int row_step, int64_t n_envs, int n_members);
int pcc_update_diag_pop(const float *act, const float *logp_old, const float *mean_new, const float *ret, const float *val, int T,
                        int row_step, int64_t n_envs, int n_members, const float *params, int64_t param_stride, int64_t log_std_index,
                        const float *hyper, double kl_limit, int epoch, double *diag, int64_t diag_stride, int32_t *stop,
                        float *hyper_live, double *scratch, void *stream);
int pcc_update_diag(const float *act, const float *logp_old, const float *mean_new, const float *ret, const float *val, int T,
                    int row_step, int64_t n_envs, const float *params, int64_t log_std_index, float clip, double *diag,
                    double *scratch, void *stream);

/*
 * Gradient-norm clipping and a non-finite guard beside the fused PPO step: one optimiser step of every
 * member as pcc_ppo_minibatch_step_pop takes it, with a global limit on the norm of each member's gradient and with a step whose
 * gradient is not finite left out.  Every argument of pcc_ppo_minibatch_step_pop in its order and with its meaning, grad_out
 * REQUIRED, then:
 * hyper_grad   float32 [n_members][8] work block, caller-owned; it must not be `hyper`
 * clip         float64 [n_members][clip_stride], clip_stride >= 8: row m is {sumsq, norm, c, state, steps, clipped_steps,
 *              skipped_steps, max_norm_seen}.  Columns 0 - 3 are overwritten by every call; columns 4 - 7 are accumulated, the caller
 *              zeroes them at the start of an update; the padding is never read or written
 * Four launches on `stream`, nothing synchronizes, no atomics:
 * 1. hyper_grad[m][0 .. 8) = hyper[m][0 .. 8) with hyper_grad[m][0] = 0.0f.
 * 2. pcc_ppo_minibatch_step_pop with hyper_grad in place of hyper -- its two launches as they are; every member is gradient-only
 *    there: grad_out holds the summed gradient G (the entropy term included) and stats_out what that call writes; params, adam_m and
 *    adam_v are untouched.
 * 3. Per member, n = n_params, g[p] = grad_out[m * param_stride + p]: 256 lanes; lane j adds (double)g[p] * (double)g[p] for p = j,
 *    j + 256, j + 512, ... < n in increasing p, from 0.0, one float64 multiply and one float64 add per term, no contraction; then
 *    the lane sums x[0 .. 256) are combined by the tree: for s = 128, 64, ..., 1: x[j] += x[j + s] for every j < s.  sumsq = x[0],
 *    norm = sqrt(sumsq).  With lr = hyper[m][0] and M = hyper[m][5] -- `hyper` is the caller's block, which may be
 *    pcc_update_diag_pop's hyper_live -- and c64 = (double)M / (norm + 1e-6), torch.nn.utils.clip_grad_norm_'s coefficient, the first
 *    of these that holds gives the member's state:
 *      lr == 0              state 3, gradient only: nothing but the row of clip is written
 *      sumsq not finite     state 2, skipped: params, adam_m and adam_v of the member keep their bits
 *      M > 0 && c64 < 1.0   state 1, clipped: c = (float)c64
 *      otherwise            state 0: c = 1.0f                             (c is reported as 1 in the states 2 and 3)
 *    In the states 0 and 1, for every p < n: gc = g[p] * c, one float32 multiply (c == 1.0f leaves g[p] exactly), then Adam on gc
 *    operation for operation as pcc_ppo_minibatch_step_pop does it on g[p], the bias corrections computed on the host as there: a
 *    step in state 0 leaves in params, adam_m and adam_v the bits pcc_ppo_minibatch_step_pop leaves.  Then steps += 1 in the states
 *    0 and 1, clipped_steps += 1 in state 1, skipped_steps += 1 in state 2, max_norm_seen = fmax(max_norm_seen, norm): a NaN norm
 *    does not enter it.  A member's results do not depend on the other members: they are bit-identical to the same call on that member
 *    alone as a population of one.
 * adam_step is the population's: it goes on for a skipped member as it does for a stopped one.
 * Returns 0; -1, with nothing written and before any device call, for everything pcc_ppo_minibatch_step_pop answers -1 to, a NULL
 * grad_out / hyper_grad / clip, hyper_grad == hyper, clip_stride < 8; -2 outside the domain of pcc_ppo_supported; -3 launch failure.
 */
int pcc_ppo_minibatch_step_clip_pop(const float *obs, const float *act, const float *logp_old, const float *adv, const float *ret,
                                    const int64_t *perm, int64_t perm_stride, int64_t start, int64_t count, int obs_dim, int h1, int h2,
                                    float *params, float *adam_m, float *adam_v, int64_t param_stride, int n_members, const float *hyper,
                                    int adam_step, float beta1, float beta2, float eps, float *scratch, float *grad_out, float *stats_out,
                                    float *hyper_grad, double *clip, int64_t clip_stride, void *stream);

/*
 * Keyed random streams of a learner and the standardisation of its advantages: everything a PPO iteration
 * draws, as a pure function of (the learner's 64-bit key, iteration, step or epoch, the learner's LOCAL sample index) -- never of
 * the member's index, of n_envs or n_members other than through n_m = n_envs / n_members, or of any generator's state.  Member m
 * owns the columns [m * n_m, (m + 1) * n_m) of every [T][n_envs] row, as above; its local env e is column m * n_m + e.  keys: device
 * uint64 [n_members].  The Philox block of (c0, c1, c2, c3) under a key is Philox4x32-10 (Salmon et al. 2011) with the counter
 * words c0 .. c3 and the key words {key & 0xffffffff, key >> 32}; its output words are w0 .. w3.  All buffers are caller-owned device
 * memory; everything is enqueued on `stream`, nothing synchronizes; no atomics.
 *
 * pcc_rollout_noise_pop, one launch: noise_out [T][n_envs] float32 standard normals.  The local envs 4 q .. 4 q + 3 of step t share
 * the block of (q, t, iteration, 0x4E4F4953) under keys[m].  In float64: u1 = ((double)w0 + 1) / 2^32, in (0, 1], so the logarithm is
 * finite; r = sqrt(-2 log(u1)); env 4 q gets r cos(2 pi w1 / 2^32), env 4 q + 1 gets r sin(2 pi w1 / 2^32); the envs 4 q + 2 and
 * 4 q + 3 the same from (w2, w3) in place of (w0, w1).  The products are rounded to float32 once.  The device's float64 log, sqrt and
 * sincospi are good to a few units of the last float64 place, so a value is the correctly rounded one or, rarely, its float32
 * neighbour; |z| <= sqrt(64 log 2) = 6.67.  words_out: NULL, or uint32 [T][n_envs]: the word w(e & 3) of every env's block, for
 * tests of this layout.
 *
 * pcc_sample_order_pop, one launch: row m of perm_out [n_members][perm_stride] int64 is a permutation of member m's own n = T * n_m
 * samples, as the global indices t * n_envs + m * n_m + e pcc_ppo_minibatch_step_pop reads; the padding perm_stride - n is never
 * written.  No sort: position i holds the local sample j = t * n_m + e that a keyed bijection sends i to.  With h the smallest
 * integer with 4^h >= n and mask = 2^h - 1, F is the balanced Feistel network of 6 rounds on the 2 h bit values x = (L << h) | R:
 * per round r = 0 .. 5, (L, R) <- (R, L ^ (fmix32(R + k_r) & mask)), the sum in 32 bits, fmix32 the 32-bit finaliser of MurmurHash3
 * (v ^= v >> 16, v *= 0x85EBCA6B, v ^= v >> 13, v *= 0xC2B2AE35, v ^= v >> 16), k_r = w(r & 3) + r * 0x9E3779B9 in 32 bits from the
 * block of (epoch, 0, iteration, 0x4F524452) under keys[m].  j is the first of F(i), F(F(i)), ... below n (cycle walking: the walk
 * follows a cycle of a permutation of [0, 4^h) that starts at i < n, so it ends; 4^h < 4 n, so a walk takes fewer than 4
 * evaluations on average).  The local permutation depends on (key, iteration, epoch, n) only.
 *
 * pcc_adv_standardise_pop, three launches: out [T][n_envs] = float32((a - mean) / (sqrt(var) + 1e-8)) per member over its own n = T *
 * n_m values a = (double)adv[t][column], float64 throughout: mean = S1 / n, S1 the sum of a; var = S2 / (n - 1), S2 the sum of
 * (a - mean) * (a - mean) (two passes; n = 1 gives 0 / 0: NaN, as torch's std does); moments_out float64 [n_members][2] = {mean,
 * var}.  out == adv is allowed.  Both sums are added in this order, which depends on T and n_m alone: lane = local env adds its T
 * terms in step order from 0.0; the 64 lanes of a wavefront (local envs 64 v .. 64 v + 63; lanes past n_m hold 0.0) by the tree x[j]
 * += x[j + d] for j < d, d = 32, 16, ..., 1; a workgroup of 256 lanes its four wavefronts' sums in index order; then the G = ceil(n_m /
 * 256) workgroup sums: sub-lane j of 256 adds those of index [j p, j p + p), p = ceil(G / 256), in index order from 0.0, and the
 * sub-lanes' sums by the tree x[j] += x[j + s] for j < s, s = 128, 64, ..., 1.  scratch: pcc_adv_standardise_scratch_doubles(T,
 * n_envs, n_members) doubles (host only; -1 outside the domain).
 *
 * A member's noise, order, moments and out are bit-identical to the stand-alone call with its key on a contiguous copy of its
 * columns (a member is cut into workgroups exactly as a launch over the member alone; no divisibility is asked of the member size).
 * pcc_rollout_noise / pcc_sample_order / pcc_adv_standardise are the stand-alone forms: the same kernels with one member, the key as
 * an argument, perm_out [T * n_envs], moments_out [2].
 * Returns 0; -1, with nothing written and before any device call, outside T >= 1, n_envs >= 1, 1 <= n_members <= 1024, n_envs %
 * n_members == 0, n_m < 2^31, perm_stride >= T * n_m, or for a NULL noise_out / perm_out / keys / adv / scratch / moments_out / out;
 * -3 launch failure.
 */
int pcc_rollout_noise_pop(float *noise_out, uint32_t *words_out, int T, int64_t n_envs, int n_members, const uint64_t *keys,
                          uint32_t iteration, void *stream);
int pcc_sample_order_pop(int64_t *perm_out, int64_t perm_stride, int T, int64_t n_envs, int n_members, const uint64_t *keys,
                         uint32_t iteration, uint32_t epoch, void *stream);
int pcc_adv_standardise_scratch_doubles(int T, int64_t n_envs, int n_members);
int pcc_adv_standardise_pop(const float *adv, int T, int64_t n_envs, int n_members, double *scratch, double *moments_out, float *out,
                            void *stream);
int pcc_rollout_noise(float *noise_out, uint32_t *words_out, int T, int64_t n_envs, uint64_t key, uint32_t iteration, void *stream);
int pcc_sample_order(int64_t *perm_out, int T, int64_t n_envs, uint64_t key, uint32_t iteration, uint32_t epoch, void *stream);
int pcc_adv_standardise(const float *adv, int T, int64_t n_envs, double *scratch, double *moments_out, float *out, void *stream);

/*
 * Time-limit bootstrapping: every done of this env is a truncation at max_steps, so the advantage estimation
 * may bootstrap from the value of the observation the episode ended in.  With auto-reset that observation is never written -- the
 * finishing env's row holds the next episode's empty history -- but a rollout's own rows hold all of it.  All buffers are caller-owned
 * device memory (cols and scales: host memory, read before the call returns); everything is enqueued on `stream`, nothing
 * synchronizes; no atomics: the same inputs give the same bits.  One sender per env.
 *
 * pcc_terminal_obs, one launch.
 * obs       float32 [T + 1][n_envs][H * F], oldest monitor interval first: the rows the env wrote (row t: before step t); row T is
 *           not read
 * steps     float64 [T][n_envs][19]: the step records (include/pcc_sim.h: PCC_STEP_COLS)
 * done      uint8 [T][n_envs]
 * cols, scales   [F]: feature f of the newest monitor interval is (float)(steps[t][i][cols[f]] / scales[f]), a float64 division
 *           rounded to float32 once -- for the env's feature id: column 7 + id and pcc_metric_info's scale
 * term_obs_out   float32 [n_slots][n_envs][H * F]; term_count_out int32 [n_envs]
 * The k-th done of env i in order of t (k = 0, 1, ...), at step t, fills term_obs_out[k][i] with obs[t][i][F .. H * F) followed by
 * the F new features: bit for bit the observation the env would have shown after that step without the reset.  A slot k >= the env's
 * number of dones is written as zeros; term_count_out[i] = the number of dones of env i, those beyond n_slots included (they are
 * counted, not stored).  Every element of both outputs is written.
 * Returns 0; -1, with nothing written and before any device call, for a NULL pointer, T < 1, n_envs < 1, n_slots < 1, H < 1, F
 * outside 1 .. 16, a column outside 0 .. 18, a scale that is not finite and > 0; -3 launch failure.
 *
 * pcc_gae_boot, one launch: pcc_gae -- the same operations in the same order -- but at a done at (t, i) delta = rewards + gamma *
 * v_term - values and the running sum restarts at delta (the recursion is still cut), v_term = term_value[slot][i], slot = the
 * number of dones of env i in the rows below t, or 0 for slot >= n_slots (pcc_gae's result).  term_value float32 [n_slots][n_envs]:
 * the value of term_obs_out[slot][i] (pcc_policy_act_pop with noise == NULL on each slot's rows, value_out alone); term_count int32
 * [n_envs]: pcc_terminal_obs's counts of the same done rows.  On an env without a done the outputs are bit-identical to pcc_gae's.
 * pcc_gae_boot_pop: gamma and lambda per member from hyper, as pcc_gae_pop; a member's outputs are bit-identical to pcc_gae_boot on a
 * contiguous copy of its columns.
 * Return 0; -1, with nothing written and before any device call, for a NULL pointer, T < 1, n_envs < 1, n_slots < 1, n_members
 * outside 1 .. 1024, n_envs % n_members != 0; -3 launch failure.
 */
int pcc_terminal_obs(const float *obs, const double *steps, const uint8_t *done, int T, int64_t n_envs, int H, int F,
                     const int32_t *cols, const double *scales, int n_slots, float *term_obs_out, int32_t *term_count_out, void *stream);
int pcc_gae_boot(const float *rewards, const float *values, const uint8_t *dones, const float *last_value, const float *term_value,
                 const int32_t *term_count, int n_slots, int T, int64_t n_envs, float gamma, float lam, float *adv_out, float *ret_out,
                 void *stream);
int pcc_gae_boot_pop(const float *rewards, const float *values, const uint8_t *dones, const float *last_value, const float *term_value,
                     const int32_t *term_count, int n_slots, int T, int64_t n_envs, int n_members, const float *hyper, float *adv_out,
                     float *ret_out, void *stream);

/*
 * Reward objectives: the reward rows of a rollout recomputed from its step records under per-member weights
 * over six of their metrics.  The env's own reward is the fixed combination (10 recv_rate / 12000 - 1e3 avg_latency - 2e3 loss_ratio)
 * 1e-3; every metric it is made of is in the float64 step record, so another combination needs no env kernel.  All buffers are
 * caller-owned device memory; everything is enqueued on `stream`, nothing synchronizes; no atomics: the same inputs give the same
 * bits.  One sender per env.
 * steps       float64 [T][n_envs][PCC_STEP_COLS] (include/pcc_sim.h): m[X] below is column PCC_COL_METRIC0 + PCC_M_X of a record
 * weights     float64 [n_members][PCC_OBJ_TERMS]: member m owns the columns [m * n_m, (m + 1) * n_m) of every row, n_m = n_envs /
 *             n_members, and its row of weights holds for them; the caller keeps them finite
 * reward_out  float32 [T][n_envs]
 * sums        float64 [n_members][PCC_OBJ_TERMS + 1], or NULL (then the second launch is left out)
 * scratch     pcc_objective_scratch_doubles(T, n_envs, n_members) doubles (host only; -1 outside the domain)
 * The reward of a sample, in float64: the terms of the enum below in index order, a term whose weight is exactly 0 left out -- its
 * metric is never read, so an unused column cannot make the reward NaN; the first term that is not left out starts the sum, every
 * later one is added to it; the sum times 1e-3 (the env's kRewardScale), rounded to float32 once.  No term at all gives 0.0f.  One
 * multiply, one divide and one add per operation written, no contraction: with the weights (10, -1e3, -2e3, 0, 0, 0) reward_out holds
 * the bits of the env's own reward rows, and of (float)steps[..][PCC_COL_REWARD].
 * sums[m][k], k < PCC_OBJ_TERMS, is the sum over the member's T * n_m samples of weighted term k before the scale (0 for a term left
 * out), sums[m][PCC_OBJ_TERMS] that of the float32 rewards widened to float64.  Every sum is added in this order, which depends on T
 * and n_m alone: lane = local env adds its T values in step order from +0.0; the 64 lanes of a wavefront (local envs 64 v .. 64 v +
 * 63; lanes past n_m hold 0.0) by the tree x[j] += x[j + d] for j < d, d = 32, 16, ..., 1; a workgroup of 256 lanes its four
 * wavefronts' sums in index order; then the G = ceil(n_m / 256) workgroup sums: sub-lane j of 256 adds those of index [j p, j p + p),
 * p = ceil(G / 256), in index order from 0.0, and the sub-lanes' sums by the tree x[j] += x[j + s] for j < s, s = 128, 64, ..., 1.
 * A member's rewards and sums are bit-identical to the stand-alone call with its weights on a contiguous copy of its columns (a
 * member is cut into workgroups exactly as a launch over the member alone; no divisibility is asked of the member size).
 * pcc_reward_objective is the stand-alone form: the same kernels with one member, weights [PCC_OBJ_TERMS], sums [PCC_OBJ_TERMS + 1].
 * Returns 0; -1, with nothing written and before any device call, for a NULL steps / weights / reward_out / scratch, T < 1, n_envs <
 * 1, n_members outside 1 .. 1024, n_envs % n_members != 0, or T * n_envs records beyond what a 64-bit byte offset holds; -3 launch
 * failure.
 */
enum {
    PCC_OBJ_THROUGHPUT = 0,     /* (w * m[RECV_RATE]) / 12000.0   packets/s */
    PCC_OBJ_LATENCY,            /*  w * m[AVG_LATENCY]            seconds   */
    PCC_OBJ_LOSS,               /*  w * m[LOSS_RATIO]                       */
    PCC_OBJ_LATENCY_INFLATION,  /*  w * m[SENT_LATENCY_INFLATION]           */
    PCC_OBJ_LATENCY_RATIO,      /*  w * m[LATENCY_RATIO]                    */
    PCC_OBJ_SEND_RATE,          /* (w * m[SEND_RATE]) / 12000.0             */
    PCC_OBJ_TERMS
};
int pcc_objective_scratch_doubles(int T, int64_t n_envs, int n_members);
int pcc_reward_objective_pop(const double *steps, int T, int64_t n_envs, int n_members, const double *weights, float *reward_out,
                             double *sums, double *scratch, void *stream);
int pcc_reward_objective(const double *steps, int T, int64_t n_envs, const double *weights, float *reward_out, double *sums,
                         double *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PCC_POLICY_H */
