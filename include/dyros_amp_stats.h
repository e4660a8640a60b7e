/* dyros_amp_stats.h -- C-ABI of TocabiAMPLower's on-GPU episode statistics (isaacgymdyros_amd/csrc/dw_amp_stats.hip).
 *
 * Opt-in (cfg sim.mi355.amp_episode_stats).  One launch after every step on the step's stream reads what the step left.  TocabiAMPLower resets
 * in reset_done(), after the step, so reset_buf, progress_buf, contact_forces, root_states, rigid_body_pos, commands, rew_buf and reward_values
 * all still belong to the episode that ends, and every term of the step's termination test is recomputed from them:
 *   DWE_C_TIME     1   (float)p >= max_episode_length - 1, p = progress_buf after the step's increment
 * and, only with enable_early_termination and p > 1,
 *   DWE_C_CONTACT  2   a COMPONENT of contact_forces[e, b, :] is > 1 for a body b other than Gym rows 8 / 16 (the soles)
 *   DWE_C_LOW      4   root_states[e, 2] < termination_height
 *   DWE_C_FLY      8   rigid_body_pos[e, 8, 2] > 0.5 or rigid_body_pos[e, 16, 2] > 0.5
 *   DWE_C_TILT     16  |quat_err(root quaternion)| > (float)(3.141592 / 4)
 * cause[e] is the OR of the bits: a pure function of this step's buffers.  Nothing here allocates, synchronises with the host or is refused by
 * a graph capture.
 *
 * Episode bookkeeping, per env, with no hook in any reset path (st words; p as above), tested in this order:
 *   1. closed, an episode on record (n >= 0) and p == previous + 1: the caller did not reset an ended env: unreset_steps, nothing else
 *   2. closed, or n < 0, or p != previous + 1: a new episode starts with this step; one that was running and not closed was interrupted from
 *      outside and counts as discarded
 *   3. this step's samples are added (none of the float ones if a word of the env's root_states row is not finite: nonfinite_steps)
 *   4. reset_buf != 0 closes the episode and folds it into the window: length p, the cause mask, the bodies if CONTACT, its return
 *
 * Caller-owned device buffers, all zero-initialised once, then DWE_ST_N filled with -1:
 *   st  [DWE_ST_WORDS][N]  32-bit words: the running episode of every env (int and float words, see DWE_ST_*)
 *   ac  [DWE_AC_WORDS][N]  float: the window's per-env sums (reduced by dwe_summarize in a fixed order)
 *   ct  [DWE_CT_WORDS]     uint64: integer counts (atomics); words [0, DWE_CT_WINDOW) belong to the window, the rest to the object's life
 *   cause [N]              uint8: this step's mask
 * A window is cleared by zeroing `ac` and ct[0, DWE_CT_WINDOW).  Setting DWE_ST_N of an env to -1 forgets its running episode.
 * Every function enqueues on `stream` and returns 0, or -1 with dwe_last_error() set. */
#ifndef DYROS_AMP_STATS_H
#define DYROS_AMP_STATS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWE_ABI_VERSION 1

#define DWE_C_TIME     1
#define DWE_C_CONTACT  2
#define DWE_C_LOW      4
#define DWE_C_FLY      8
#define DWE_C_TILT     16
#define DWE_MASKS      32    /* every combination of the five bits */

#define DWE_BODIES     38
#define DWE_LFOOT      8     /* Gym rows of L_Foot_Link / R_Foot_Link (env.contactBodies) */
#define DWE_RFOOT      16
#define DWE_LEN_BINS   16    /* episode-length histogram over [0, max_episode_length] */
#define DWE_CMD_BINS   4     /* commands[0] over the cfg's command.x range, per step  */
#define DWE_REW_TERMS  9     /* reward_values                                         */

/* st: int words */
#define DWE_ST_N       0     /* samples of the running episode; -1: none running   */
#define DWE_ST_PREV    1     /* progress_buf at the previous record                */
#define DWE_ST_CLOSED  2     /* the episode on record has ended                    */
/* st: float words */
#define DWE_ST_RET     3     /* sum of rew_buf over the episode's samples          */
#define DWE_ST_PKL     4     /* peak sole F_z / (9.81 total_mass), left / right    */
#define DWE_ST_PKR     5
#define DWE_ST_WORDS   6

/* ac: float sums of the window, per env */
#define DWE_AC_RET     0     /* return of finished episodes                        */
#define DWE_AC_REW     1     /* [9] reward_values per step                         */
#define DWE_AC_VERR    10    /* [4] per command bin: |commands[0] - local v_x| per step */
#define DWE_AC_VCNT    14    /* [4]   steps in the bin                             */
#define DWE_AC_YAW     18    /* |commands[2] - root_states[12]| per step           */
#define DWE_AC_PK      19    /* [2] per-episode sole peaks                         */
#define DWE_AC_WORDS   21

/* ct: uint64 counts */
#define DWE_CT_RECORDS    0  /* records in the window                              */
#define DWE_CT_EPISODES   1
#define DWE_CT_DISCARDED  2  /* running episodes interrupted by an outside reset   */
#define DWE_CT_UNRESET    3  /* steps of ended envs the caller did not reset       */
#define DWE_CT_NONFINITE  4  /* steps whose root_states row is not finite          */
#define DWE_CT_SAMPLES    5  /* steps that added to the float sums                 */
#define DWE_CT_MASK       6  /* [32] finished episodes by cause mask               */
#define DWE_CT_LEN_SUM    38
#define DWE_CT_LEN_MAX    39
#define DWE_CT_LEN_HIST   40 /* [16]                                               */
#define DWE_CT_BODY       56 /* [38] bodies with a component > 1 at a CONTACT end  */
#define DWE_CT_SOLE_OVER  94 /* [2] sampled steps with sole F_z > 1.4 * 9.81 * total_mass */
#define DWE_CT_WINDOW     96
#define DWE_CT_CALLS      96 /* records since construction                         */
#define DWE_CT_WORDS      97

/* dwe_summarize's output: doubles, ct as they are, then the sums of ac */
#define DWE_SUM_AC        DWE_CT_WORDS
#define DWE_SUM_WORDS     (DWE_CT_WORDS + DWE_AC_WORDS)

int dwe_abi_version(void);
const char *dwe_last_error(void);
/* after a step: cause[N], st, ac and ct updated from the step's buffers (root_states [N,13], contact_forces [N,38,3], rigid_body_pos [N,38,3],
 * commands [N,3], rew_buf [N], reward_values [N,9], reset_buf / progress_buf [N] int64, total_mass [N]); command_x_lo / _hi: the cfg's
 * command.x range */
int dwe_record(int32_t num_envs, const float *root_states, const float *contact_forces, const float *rigid_body_pos, const float *commands,
               const float *rew_buf, const float *reward_values, const int64_t *reset_buf, const int64_t *progress_buf, const float *total_mass,
               void *st, float *ac, uint64_t *ct, uint8_t *cause, float max_episode_length, float termination_height,
               int32_t enable_early_termination, float command_x_lo, float command_x_hi, void *stream);
/* out [DWE_SUM_WORDS] doubles: one workgroup per float word, every sum in a fixed order */
int dwe_summarize(int32_t num_envs, const float *ac, const uint64_t *ct, double *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
