/* dyros_meter.h -- C-ABI of the learners' on-GPU episode-return meter (isaacgymdyros_amd/csrc/dw_meter.hip).
 *
 * Learner-side and task-agnostic: it sees only (reward, done) of a step and, optionally, the stacked reward terms.  It restates what the
 * reference learner does per step with current_rewards, current_lengths and two rl_games AverageMeter objects
 * (a2c_common_dyros.py:663-684, amp_continuous.py:126-143) -- there a dones.nonzero(), a gather and a host-side update, a host sync per
 * step -- as ONE launch after env.step with no sync, no allocation and no argument that changes from call to call, so it sits inside a
 * captured rollout step.
 *
 * Caller-owned device buffers, zero-initialised once:
 *   cur  [C + 1][N] float            the running episode of every env: C return columns, then the length.  Column-major: a wavefront's
 *                                    loads of one column are consecutive words
 *   ms   [DWM_MS_WORDS] 32-bit words the meter state (DWM_MS_*), 8-byte aligned
 *   work [dwm_work_words(N, C)] 32-bit words: DWM_WORK_HEAD words whose first is the ticket, then one partial row of C + 3 words per
 *                                    workgroup of DWM_GROUP envs: C return sums, the length sum (float), the count of D and the count of
 *                                    discarded games (uint32)
 * Column 0 is the step reward rew [N]; columns 1 .. C-1 are the first C-1 columns of stacked [N][stacked_stride] (NULL: C must be 1).
 * done is [N] int64, as VecTask.reset_buf.
 *
 * One dwm_record, exactly (fp32 unless said otherwise; built with -ffp-contract=off):
 *   cur[c][i] += (rew, stacked[:, :C-1])[c][i] for c < C;  cur[C][i] += 1
 *   D = {i : done[i] != 0 and every cur[c][i], c < C, is finite};  k = |D|
 *   if k > 0:
 *       new_mean[c] = (sum over D of cur[c][i]) / (float)k                      c = 0 .. C, the length included
 *       size = min(k, max_size);  old = min(max_size - size, current_size)
 *       mean[c] = (mean[c] * (float)old + new_mean[c] * (float)size) / (float)(old + size)            in this order
 *       current_size = old + size
 *       games += k;  sum_ret += sum over D of cur[0];  sum_len += sum over D of cur[C]        (double, see below)
 *   discarded += |{i : done[i] != 0} \ D|
 *   cur[:, i] = 0 for every i with done[i] != 0
 * This is AverageMeter.update(current_rewards[done_indices]) followed by the multiplication with not_dones, with ONE deliberate
 * difference: a finished episode whose return is not finite in some column is discarded and counted, not averaged.  The step kernel's
 * non-finite guard resets such an env, and one NaN must not poison a meter for the rest of a run.
 *
 * The order of every sum is fixed, so the result is a defined function of the inputs:
 *   1. Env i belongs to workgroup i / DWM_GROUP, wavefront (i % DWM_GROUP) / 64, lane i % 64.  An env outside D, or past N, adds +0.0f.
 *   2. Inside a wavefront the 64 terms of a column are added as the xor butterfly does: t[l] = t[l] + t[l ^ 32], then ^ 16, 8, 4, 2, 1
 *      (a binary tree of depth 6: lane l first meets lane l + 32).
 *   3. The workgroup's sum is ((w0 + w1) + w2) + w3 over its four wavefronts; it is the partial row.
 *   4. The totals are the partial rows added one by one in workgroup-index order, starting from +0.0f (counts: uint32).  sum_ret and
 *      sum_len add the same partial rows of column 0 and column C in the same order in double, starting from 0.0, and that total is
 *      added to the stored double.
 * The workgroup that adds the rows is the one whose agent-scope acquire-release increment of the ticket, made after its partial row is
 * released, returns the last number; it sets the ticket back to zero, so a graph replay starts clean.  No workgroup waits for another.
 * Every function enqueues on `stream` and returns 0, or -1 with dwm_last_error() set. */
#ifndef DYROS_METER_H
#define DYROS_METER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWM_ABI_VERSION 1

#define DWM_COLS_MAX  16    /* return columns: the step reward and up to 15 reward terms */
#define DWM_GROUP     256   /* envs per workgroup */
#define DWM_WORK_HEAD 4     /* words of `work` before the partial rows; word 0 is the ticket */

/* ms: 32-bit words */
#define DWM_MS_CURRENT_SIZE 0    /* uint32: games in the window, at most max_size */
#define DWM_MS_MEAN         2    /* float [DWM_COLS_MAX]: the window's mean return per column */
#define DWM_MS_MEAN_LEN     18   /* float: the window's mean episode length */
#define DWM_MS_GAMES        20   /* uint64: games averaged since the last clear */
#define DWM_MS_DISCARDED    22   /* uint64: finished games with a non-finite return since the last clear */
#define DWM_MS_SUM_RET      24   /* double: sum of column 0 over those games */
#define DWM_MS_SUM_LEN      26   /* double: sum of their lengths */
#define DWM_MS_WORDS        28

int dwm_abi_version(void);
const char *dwm_last_error(void);
/* 32-bit words of `work` for num_envs envs and cols columns; -1 for arguments dwm_record refuses */
int64_t dwm_work_words(int32_t num_envs, int32_t cols);
/* after a step: see above.  1 <= cols <= DWM_COLS_MAX, max_size >= 1, stacked_stride >= cols - 1 */
int dwm_record(int32_t num_envs, int32_t cols, int32_t max_size, const float *rew, const float *stacked, int32_t stacked_stride,
               const int64_t *done, float *cur, void *ms, void *work, void *stream);
/* AverageMeter.clear() and the totals: zeroes ms and the head of work (the running episodes in cur go on) */
int dwm_clear(void *ms, void *work, void *stream);

#ifdef __cplusplus
}
#endif

#endif
