/* dyros_gait.h -- C-ABI of DyrosDynamicWalk's on-GPU gait profile (isaacgymdyros_amd/csrc/dw_gait.hip).
 *
 * Opt-in (cfg sim.mi355.gait_profile).  One launch after every step on the step's stream reads what the step left and adds every env's
 * sample to the row of its mocap phase bin:
 *   bin = DW_ES_MOCAP_IDX / (3600 / B),  B one of {12, 24, 36, 72, 144}
 * The index runs 0 .. 3598 (the step kernel takes it modulo 3599); with these B the reward's window edges 300, 1500, 2100 and 3300 fall on
 * bin edges, so every bin lies in one window: DWG_WIN_DSP [3300, 3600) + [0, 300) + [1500, 2100), DWG_WIN_RSSP [300, 1500), DWG_WIN_LSSP
 * [2100, 3300).  Nothing here allocates, synchronises with the host or takes an argument that changes from call to call, so dwg_record
 * sits inside a captured rollout step.
 *
 * Which env-steps count.  The step kernel resets an env in the launch that ends its episode.  Such an in-step reset leaves DW_ES_MOCAP_IDX,
 * DW_ES_TARGET_FORCE, DW_ES_TARGET_QPOS, contact_forces and action_torque as the terminal step's, while root_states, dof_state,
 * DW_ES_PERT_ON, DW_ES_TARGET_VEL and progress_buf (= 0) already belong to the new episode: the row would mix two episodes.  Hence, tested in
 * this order, an env-step
 *   with reset_buf != 0                                          adds nothing and is counted in DWG_CT_SKIPPED_TERMINAL
 *   with progress_buf < min_episode_step,
 *     or with DW_ES_PERT_ON set while skip_pushes != 0           adds nothing and is counted in DWG_CT_SKIPPED_FILTER
 *   with a non-finite word among those read (below), or with
 *     DW_ES_MOCAP_IDX outside [0, 3600)                          adds nothing and is counted in DWG_CT_DISCARDED
 * and every other env-step is added and counted in DWG_CT_RECORDED.  The four counts of one record add up to num_envs.
 *
 * The words read: z of the contact_forces rows DWS_LFOOT / DWS_RFOOT (8 / 16), total_mass, DW_ES_TARGET_FORCE [2], root_states words 2 and
 * 7, DW_ES_TARGET_VEL [0], dof_pos and DW_ES_TARGET_QPOS of the 12 leg joints (DOF 0 .. 11; dof_state is [N][33][2], position first),
 * DW_ES_ACTION_TORQUE [12] and column DWG_PAID_COLUMN of stacked_rewards.
 *
 * A row is DWG_W 64-bit signed sums (fp32 expressions as dw_stats.h forms them, built with -ffp-contract=off):
 *    0      count of env-steps
 *    1, 2   F_z of the left / right sole
 *    3, 4   F_z * F_z (formed in double)
 *    5, 6   expected F_z = -(ws * target_force), ws = total_mass / 104.48f
 *    7, 8   fabsf(F_z + ws * target_force)
 *    9, 10  counts of F_z > 1.0f (the reward's lcon / rcon)
 *   11      count of stacked_rewards[DWG_PAID_COLUMN] > 0: the step kernel paid foot_contact_reward
 *   12      count of steps the recorder's own rule pays: the window of the bin with lcon / rcon (DSP both, RSSP right only, LSSP left only)
 *   13      root z (root_states[2])
 *   14      root_states[7] - target_vel[0]
 *   15      count of steps with DW_ES_PERT_ON set
 *   16..27  fabsf(dof_pos - target_qpos) of the 12 leg joints
 *   28..39  fabsf(action_torque) of the 12 leg joints
 * A count adds 1.  A sample v adds llrint(clamp((double)v, -2^30, 2^30) * 65536.0), round to nearest even (DWG_FRAC_BITS fraction bits);
 * the squares are clamped after squaring.  Integer addition does not depend on its order: a summary is the same bits from run to run and
 * between eager and replayed steps, and equals a numpy restatement exactly.  No floating-point atomic is used.  One add is at most 2^46 in
 * magnitude, so a word cannot overflow before 2^17 adds to one bin, and not before 2^63 / (|v| * 65536) adds of samples of size |v|
 * (a squared sole force of 1000 N: 2^27 env-steps in one bin).
 *
 * Caller-owned device buffers, zeroed once (or by dwg_clear):
 *   part [dwg_groups(N)][B][DWG_W] int64  one partial table per workgroup of DWG_GROUP envs; only its workgroup writes it
 *   ct   [DWG_CT_WORDS] int64             the counters
 *   out  [B * DWG_W + DWG_CT_WORDS] int64 dwg_summarize's result: the table, then the counters
 * Every function enqueues on `stream` and returns 0, or -1 with dwg_last_error() set. */
#ifndef DYROS_GAIT_H
#define DYROS_GAIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWG_ABI_VERSION 1

#define DWG_W            40    /* words of a row */
#define DWG_BINS_MAX     144
#define DWG_BINS_DEFAULT 72
#define DWG_ROWS         3600  /* mocap rows a cycle is binned over */
#define DWG_GROUP        64    /* envs per workgroup and partial table */
#define DWG_FRAC_BITS    16
#define DWG_CLAMP_LOG2   30
#define DWG_LEG_JOINTS   12
#define DWG_PAID_COLUMN  8     /* foot_contact_reward in stacked_rewards [N][15] */

/* row words */
#define DWG_R_COUNT      0
#define DWG_R_FZ         1     /* [2] */
#define DWG_R_FZ2        3     /* [2] */
#define DWG_R_EXPECTED   5     /* [2] */
#define DWG_R_FERR       7     /* [2] */
#define DWG_R_CONTACT    9     /* [2] */
#define DWG_R_PAID       11
#define DWG_R_PREDICTED  12
#define DWG_R_ROOT_Z     13
#define DWG_R_VEL_ERR    14
#define DWG_R_PERT       15
#define DWG_R_JOINT_ERR  16    /* [12] */
#define DWG_R_TORQUE     28    /* [12] */

/* gait windows of the reward (dw_oct_post.h) */
#define DWG_WIN_DSP      0
#define DWG_WIN_RSSP     1
#define DWG_WIN_LSSP     2

/* ct */
#define DWG_CT_RECORDED         0
#define DWG_CT_SKIPPED_TERMINAL 1
#define DWG_CT_SKIPPED_FILTER   2
#define DWG_CT_DISCARDED        3
#define DWG_CT_WORDS            4

int dwg_abi_version(void);
const char *dwg_last_error(void);
/* workgroups (partial tables) of num_envs envs; -1 for num_envs < 1 */
int64_t dwg_groups(int32_t num_envs);
/* after a step: root_states [N,13], dof_state [N,33,2], contact_forces [N,38,3], env_state [N,DW_ES_WORDS], stacked_rewards [N,15],
 * reset_buf and progress_buf [N] int64, total_mass [N] */
int dwg_record(int32_t num_envs, int32_t bins, int32_t min_episode_step, int32_t skip_pushes, const float *root_states, const float *dof_state,
               const float *contact_forces, const float *env_state, const float *stacked_rewards, const int64_t *reset_buf,
               const int64_t *progress_buf, const float *total_mass, int64_t *part, int64_t *ct, void *stream);
/* a new window: zeroes part and ct */
int dwg_clear(int32_t num_envs, int32_t bins, int64_t *part, int64_t *ct, void *stream);
/* out = the sum of the partial tables, then ct */
int dwg_summarize(int32_t num_envs, int32_t bins, const int64_t *part, const int64_t *ct, int64_t *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
