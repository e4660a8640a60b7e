/* dyros_trace.h -- C-ABI of DyrosDynamicWalk's on-GPU run trace (isaacgymdyros_amd/csrc/dw_trace.hip).
 *
 * Opt-in (cfg sim.mi355.run_trace).  A flight recorder: K chosen envs ("slots") each keep a ring of their last T steps.  One launch after
 * every step on the step's stream copies what the step left for those envs -- root_states, dof_state, contact_forces, rew_buf,
 * stacked_rewards, reset_buf, timeout_buf and spans of the env_state record (through the DW_ES_* offsets of dyros_walk.h) -- into one row
 * of DWT_ROW_WORDS 32-bit words.  A slot can be frozen ("held") at the step that ends an episode, so that its ring keeps the approach to
 * a fall until the slot is armed again.  Nothing here allocates, synchronises with the host or is refused by a graph capture, and no
 * argument of dwt_record changes from call to call.
 *
 * Caller-owned device buffers:
 *   ring     [K][T][DWT_ROW_WORDS] 32-bit words, 16-byte aligned: slot-major, one env's history is one contiguous span
 *   ss       [DWT_SS_WORDS][K]     uint32: the state of every slot (see DWT_SS_*), zero-initialised once
 *   slot_env [K] int32             the env of every slot (distinct, in [0, N))
 *   env_slot [N] int32             the slot of every env, -1 for an env that is not traced
 *
 * A record, per slot (n = the slot's own count of steps in the running episode, as DWS_ST_N of dyros_stats.h):
 *   seen += 1.  A held slot does nothing else.
 *   n1 = n + 1; the row (EPI_STEP = n1, SEEN = seen) is written to ring[slot][cursor % T]; cursor += 1.
 *   If reset_buf is set: the episode ended by its time limit if (float)n1 >= max_episode_length - 1, by a fall otherwise (falls += 1);
 *   n = 0; the slot becomes held if hold_mode is DWT_HOLD_RESET, or DWT_HOLD_FALL and it was a fall.  Otherwise n = n1.
 * So a frozen ring ends with the terminating step.
 * Every function enqueues on `stream` and returns 0, or -1 with dwt_last_error() set. */
#ifndef DYROS_TRACE_H
#define DYROS_TRACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWT_ABI_VERSION 1

#define DWT_HOLD_NEVER 0
#define DWT_HOLD_FALL  1   /* hold at a reset that is not a time limit */
#define DWT_HOLD_RESET 2   /* hold at every reset                      */

/* the row: offsets (DWT_CH_*) and lengths (DWT_LEN_*) in 32-bit words; the spans tile [0, DWT_ROW_WORDS) in this order */
/* integer words */
#define DWT_CH_SEEN          0    /* record calls of the slot since it was armed, this one included (held calls count) */
#define DWT_LEN_SEEN         1
#define DWT_CH_EPI_STEP      1    /* the trace's own step count within the episode, this step included */
#define DWT_LEN_EPI_STEP     1
#define DWT_CH_FLAGS         2    /* DWT_FLAG_* */
#define DWT_LEN_FLAGS        1
#define DWT_CH_NAN_RESETS    3    /* DW_ES_NAN_RESETS */
#define DWT_LEN_NAN_RESETS   1
/* float words */
#define DWT_CH_ROOT          4    /* root_states */
#define DWT_LEN_ROOT         13
#define DWT_CH_DOF_POS       17   /* dof_state[:, 0] */
#define DWT_LEN_DOF_POS      33
#define DWT_CH_DOF_VEL       50   /* dof_state[:, 1] */
#define DWT_LEN_DOF_VEL      33
#define DWT_CH_QPOS_NOISE    83   /* what the policy saw */
#define DWT_LEN_QPOS_NOISE   33
#define DWT_CH_TARGET_QPOS   116
#define DWT_LEN_TARGET_QPOS  33
#define DWT_CH_ACTIONS       149
#define DWT_LEN_ACTIONS      13
#define DWT_CH_TORQUE        162  /* action_torque */
#define DWT_LEN_TORQUE       12
#define DWT_CH_FOOT_FORCE    174  /* contact_forces rows DWS_LFOOT, DWS_RFOOT */
#define DWT_LEN_FOOT_FORCE   6
#define DWT_CH_NF_MAX        180  /* the largest |F| over all other bodies (the step kernel's norm) */
#define DWT_LEN_NF_MAX       1
#define DWT_CH_NF_BODY       181  /* that body's Gym row, as a float; the lowest row among equals */
#define DWT_LEN_NF_BODY      1
#define DWT_CH_TARGET_FORCE  182
#define DWT_LEN_TARGET_FORCE 2
#define DWT_CH_TARGET_VEL    184
#define DWT_LEN_TARGET_VEL   2
#define DWT_CH_MAGNITUDE     186
#define DWT_LEN_MAGNITUDE    1
#define DWT_CH_PHASE         187
#define DWT_LEN_PHASE        1
#define DWT_CH_TIME          188
#define DWT_LEN_TIME         1
#define DWT_CH_REW           189  /* rew_buf */
#define DWT_LEN_REW          1
#define DWT_CH_STACKED       190  /* stacked_rewards */
#define DWT_LEN_STACKED      15
#define DWT_CH_PAD           205  /* zeros */
#define DWT_LEN_PAD          3
#define DWT_ROW_WORDS        208  /* 832 bytes, a multiple of 16 */

#define DWT_FLAG_RESET       1    /* reset_buf                                              */
#define DWT_FLAG_TIME_LIMIT  2    /* (float)EPI_STEP >= max_episode_length - 1              */
#define DWT_FLAG_PERT_ON     4
#define DWT_FLAG_PERT_START  8    /* perturb_start                                          */
#define DWT_FLAG_TIMEOUT     16   /* timeout_buf                                            */

/* ss: uint32 words, per slot */
#define DWT_SS_CURSOR 0    /* rows written since the slot was armed; the next row goes to cursor % T.  A count that reaches
                            * DWT_CURSOR_FOLD (about 6 days of steps) continues from T + cursor % T: the same next row, the ring full */
#define DWT_SS_HELD   1
#define DWT_SS_N      2    /* steps of the running episode */
#define DWT_SS_SEEN   3    /* record calls since the slot was armed */
#define DWT_SS_FALLS  4    /* episodes since the slot was armed that ended other than by the time limit */
#define DWT_SS_WORDS  5
#define DWT_CURSOR_FOLD 0xfffffff0

int dwt_abi_version(void);
const char *dwt_last_error(void);
/* after a step: one row per slot that is not held (root_states [N,13], dof_state [N,33,2], contact_forces [N,38,3], env_state
 * [N,DW_ES_WORDS], rew_buf [N], stacked_rewards [N,15], reset_buf / timeout_buf [N] int64) */
int dwt_record(int32_t num_envs, int32_t num_slots, int32_t depth, int32_t hold_mode, const int32_t *slot_env, const float *root_states,
               const float *dof_state, const float *contact_forces, const float *env_state, const float *rew_buf,
               const float *stacked_rewards, const int64_t *reset_buf, const int64_t *timeout_buf, float max_episode_length, void *ss,
               void *ring, void *stream);
/* clears cursor, held, seen and falls of the slots of the listed envs (env_ids == NULL: of every traced env) and restarts their episode
 * count from progress_buf [N] int64; envs that are not traced, or out of range, are ignored */
int dwt_arm(int32_t num_envs, int32_t num_slots, const int32_t *env_ids, int32_t num_ids, const int64_t *progress_buf,
            const int32_t *env_slot, void *ss, void *stream);
/* out [num_ids][depth][DWT_ROW_WORDS] (16-byte aligned): the rows of the listed slots (slot_ids == NULL: slots 0 .. num_ids - 1), oldest
 * first, unused rows zero; out_rows [num_ids] = min(cursor, depth).  A slot id out of range gives zero rows. */
int dwt_gather(int32_t num_slots, int32_t depth, const int32_t *slot_ids, int32_t num_ids, const void *ss, const void *ring, void *out,
               int32_t *out_rows, void *stream);

#ifdef __cplusplus
}
#endif

#endif
