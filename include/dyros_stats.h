/* dyros_stats.h -- C-ABI of DyrosDynamicWalk's on-GPU episode statistics (isaacgymdyros_amd/csrc/dw_stats.hip).
 *
 * Opt-in (cfg sim.mi355.episode_stats).  One launch after every step on the step's stream reads what the step left -- reset_buf,
 * root_states, contact_forces, the env_state record (through the DW_ES_* offsets of dyros_walk.h) and total_mass -- and decides, for each
 * env that reset, why its episode ended:
 *   DWS_CAUSE_NON_FINITE       4   the env's DW_ES_NAN_RESETS is higher than at the previous record
 *   DWS_CAUSE_NON_FOOT_CONTACT 2   a body other than Gym rows 8 / 16 (the soles) has |F| > 1 N in contact_forces (the step kernel's norm)
 *   DWS_CAUSE_TIME_LIMIT       1   (float)n >= max_episode_length - 1, n = the statistics' own count of steps in the episode
 *   DWS_CAUSE_ORIENTATION      3   what is left: the only remaining term of the step kernel's OR is quat_diff_rad > 0.5
 * tested in this order (0: no reset).  Nothing here allocates, synchronises with the host or is refused by a graph capture.
 *
 * Caller-owned device buffers, all zero-initialised once:
 *   st  [DWS_ST_WORDS][N]  32-bit words: the running episode of every env (int and float words, see DWS_ST_*)
 *   ac  [DWS_AC_WORDS][N]  float: the window's per-env sums (reduced by dws_summarize in a fixed order)
 *   ct  [DWS_CT_WORDS]     uint64: integer counts (atomics); words [0, DWS_CT_WINDOW) belong to the window, the rest to the object's life
 *   cause [N]              uint8: the cause of this step, 0 for an env that did not reset
 * A window is cleared by zeroing `ac` and ct[0, DWS_CT_WINDOW).
 * Every function enqueues on `stream` and returns 0, or -1 with dws_last_error() set. */
#ifndef DYROS_STATS_H
#define DYROS_STATS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWS_ABI_VERSION 2

#define DWS_CAUSE_NONE             0
#define DWS_CAUSE_TIME_LIMIT       1
#define DWS_CAUSE_NON_FOOT_CONTACT 2
#define DWS_CAUSE_ORIENTATION      3
#define DWS_CAUSE_NON_FINITE       4

#define DWS_LFOOT        8     /* Gym rows of L_Foot_Link / R_Foot_Link (model.non_feet_idxs() is every other row) */
#define DWS_RFOOT        16
#define DWS_LEN_BINS     16    /* episode-length histogram over [0, max_episode_length]                            */
#define DWS_CMD_BINS     4     /* commanded target_vel[0] over [0, 0.8]                                            */
#define DWS_PUSH_WINDOW  250   /* an episode that ends at most this many steps after a push was last on is a push fall */
#define DWS_SOLE_LIMIT   1400.0f
#define DWS_RATIO_MIN_M  0.05f /* the distance ratio counts episodes whose commanded distance is at least this          */

/* st: int words */
#define DWS_ST_N      0    /* steps of the running episode                      */
#define DWS_ST_NAN    1    /* DW_ES_NAN_RESETS at the previous record            */
#define DWS_ST_NR     2    /* root_states samples of the episode (terminal step excluded) */
#define DWS_ST_PERT   3    /* pert_on at the previous record                     */
#define DWS_ST_OFF    4    /* records since pert_on was last seen set (DWS_OFF_NEVER: not in this episode) */
/* st: float words */
#define DWS_ST_X0     5    /* root x, y at the episode's start                   */
#define DWS_ST_Y0     6
#define DWS_ST_XL     7    /* root x, y at the last counted sample               */
#define DWS_ST_YL     8
#define DWS_ST_TV0    9    /* the episode's commanded target_vel[0]              */
#define DWS_ST_VERR   10   /* sum of |target_vel - root_states[7:9]|            */
#define DWS_ST_PKL    11   /* peak sole load F_z, left / right                   */
#define DWS_ST_PKR    12
#define DWS_ST_DTM    13   /* max |tau_t - tau_t-1| of the episode (action_torque of consecutive records) */
#define DWS_ST_TAU    14   /* [12] action_torque at the previous record (0 at an episode's start) */
#define DWS_ST_WORDS  26
#define DWS_OFF_NEVER 0x3fffffff

/* ac: float sums of the window, per env */
#define DWS_AC_RET    0    /* DW_ES_LAST_RETURN of finished episodes             */
#define DWS_AC_PK     1    /* [2] per-episode sole peaks                         */
#define DWS_AC_FT     3    /* [2] |F_z + total_mass / 104.48 * target_data_force| per step */
#define DWS_AC_TAU    5    /* sum of the 12 |action_torque| per step             */
#define DWS_AC_DTM    6    /* per-episode max |tau_t - tau_t-1|                   */
#define DWS_AC_VERR   7    /* [4] per command bin: per-episode mean velocity error */
#define DWS_AC_DRIFT  11   /* [4]   |y_last - y_start|                            */
#define DWS_AC_RATIO  15   /* [4]   (x_last - x_start) / (target_vel[0] * duration) */
#define DWS_AC_WORDS  19

/* ct: uint64 counts */
#define DWS_CT_RECORDS   0    /* records in the window                            */
#define DWS_CT_EPISODES  1
#define DWS_CT_CAUSE     2    /* [5] by cause code (word 2 + 0 stays 0)           */
#define DWS_CT_LEN_SUM   7
#define DWS_CT_LEN_MAX   8
#define DWS_CT_LEN_HIST  9    /* [16]                                             */
#define DWS_CT_BODY      25   /* [38] bodies over 1 N at a non_foot_contact end    */
#define DWS_CT_BIN_EP    63   /* [4] episodes per command bin                     */
#define DWS_CT_BIN_ROOT  67   /* [4]   ... with at least one root sample          */
#define DWS_CT_BIN_RATIO 71   /* [4]   ... whose distance ratio is defined        */
#define DWS_CT_PK_OVER   75   /* [2] episodes whose sole peak passed 1400 N       */
#define DWS_CT_PUSHES    77   /* rising edges of pert_on                          */
#define DWS_CT_PUSH_FALLS 78  /* non-time-limit ends during or <= 250 steps after a push */
#define DWS_CT_WINDOW    79
#define DWS_CT_CALLS     79   /* records since construction                       */
#define DWS_CT_GATE_AT   80   /* 1 + the record call that first saw env 0's perturb_start latched; 0: not yet */
#define DWS_CT_WORDS     81

/* dws_summarize's output: doubles, ct as they are, then the sums of ac */
#define DWS_SUM_AC       DWS_CT_WORDS
#define DWS_SUM_WORDS    (DWS_CT_WORDS + DWS_AC_WORDS)

int dws_abi_version(void);
const char *dws_last_error(void);
/* after a step: cause[N], st, ac and ct updated from the step's buffers (root_states [N,13], contact_forces [N,38,3], env_state
 * [N,DW_ES_WORDS], reset_buf [N] int64, total_mass [N]) */
int dws_record(int32_t num_envs, const float *root_states, const float *contact_forces, const float *env_state, const int64_t *reset_buf,
               const float *total_mass, void *st, float *ac, uint64_t *ct, uint8_t *cause, float max_episode_length, float dt_policy,
               void *stream);
/* discards the running episode of the listed envs (env_ids == NULL: all of them): their counters restart from progress_buf [N] int64 */
int dws_restart(int32_t num_envs, const int32_t *env_ids, int32_t num_ids, const float *root_states, const float *env_state,
                const int64_t *progress_buf, void *st, void *stream);
/* out [DWS_SUM_WORDS] doubles: one workgroup per float word, every sum in a fixed order */
int dws_summarize(int32_t num_envs, const float *ac, const uint64_t *ct, double *out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
