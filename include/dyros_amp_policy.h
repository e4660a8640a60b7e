/* dyros_amp_policy.h -- C-ABI of the on-GPU actor-critic of TocabiAMPLower's AMP learner (the policy share).
 *
 * What it replaces (reference: learning/amp_continuous.py, learning/common_agent.py, cfg/train/TocabiAMPLowerPPO.yaml):
 *   dwa_stats   the train-mode update of rl_games' RunningMeanStd: the observation normaliser (D = num_obs) and the value normaliser (D = 1)
 *   dwa_act     get_action_values in eval mode: normalised observations, both nets, a = mu + exp(logstd) noise, clamp(a, -1, 1), neglogp(a),
 *               the value unnormalised (ActorCritic.unnorm_value)
 *   dwa_critic  _eval_critic for the bootstrap: the critic only, unnormalised, times (1 - terminate)
 *   dwa_grad    the policy share of calc_gradients (amp_continuous.py:260-329, common_agent.py:427-511) for one minibatch: clipped surrogate,
 *               critic loss, soft bound loss, backward to every parameter
 *   dwa_opt     the optimiser step (torch.optim.Adam, betas 0.9 / 0.999, eps 1e-8, no weight decay, no clipping), then g = 0
 *   dwa_gae     common_agent.discount_values with mb_next_values, the same fp32 operations in the same order per element
 *   dwa_play    the player's get_action in eval mode (learning/common_player.py, amp_players.py): the actor only, deterministic or sampled,
 *               clamped to the +-1 action space
 * The nets: x [D] -> relu(W1 x + b1) [512] -> relu(W2 h1 + b2) [512] -> mu [A] (actor) / value [1] (critic); fp32 throughout, the
 * products on the matrix cores (v_mfma_f32_16x16x4_f32).  All pointers are device pointers; every function enqueues on `stream` and
 * returns 0, or -1 with dwa_last_error() set.  No function allocates, synchronises with the host or reads anything but its arguments, so
 * every launch can be captured in a graph and replayed; every reduction has a fixed order, so a replay gives the bits of the eager calls.
 *
 * Parameter layout (fp32, `p`; the gradient `g` and the Adam moments `m`, `v` have the same layout), D = num_obs, A = num_actions, H = 512:
 *   actor  W1 [H][D] | b1 [H] | W2 [H][H] | b2 [H] | mu W [A][H] | mu b [A]
 *   critic W1 [H][D] | b1 [H] | W2 [H][H] | b2 [H] | value w [H] | value b [1]                    (DWA_NP(D, A) floats; rows = outputs)
 * Running statistics (fp64, as rl_games keeps them): mean [D] | var [D] | count [1]                 (DWA_NSTATS(D) doubles)
 * D is 1 .. DWA_D_MAX and A is 1 .. DWA_A_MAX; the kernels pad internally. */
#ifndef DYROS_AMP_POLICY_H
#define DYROS_AMP_POLICY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWA_ABI_VERSION 2
#define DWA_HID       512   /* cfg/train/TocabiAMPLowerPPO.yaml network.mlp.units [512, 512]: the only width accepted */
#define DWA_D_MAX     512
#define DWA_A_MAX     16
#define DWA_NET(D)    ((D) * DWA_HID + DWA_HID + DWA_HID * DWA_HID + DWA_HID)
#define DWA_NP(D, A)  (DWA_NET(D) + (A) * DWA_HID + (A) + DWA_NET(D) + DWA_HID + 1)
#define DWA_NSTATS(D) (2 * (D) + 1)

/* float words of `state` (device memory, zeroed by the caller): dwa_grad ADDS one minibatch's values, the caller divides by S_UPDATES */
#define DWA_S_A_LOSS      0   /* the clipped surrogate, mean over the rows                                     */
#define DWA_S_C_LOSS      1   /* mean((ret_n - v)^2)                                                           */
#define DWA_S_B_LOSS      2   /* the soft bound 1.0, summed over the actions, mean over the rows               */
#define DWA_S_CLIP_FRAC   3   /* fraction of rows with |ratio - 1| > e_clip                                    */
#define DWA_S_UPDATES     4   /* minibatches accumulated                                                       */
#define DWA_S_LR          12  /* Adam: learning rate (the caller's schedule writes it)                         */
#define DWA_S_STEP        13  /* Adam: steps taken                                                             */
#define DWA_S_WORDS       16

typedef struct DwaLoss {            /* the yaml's coefficients */
    float e_clip;                   /* 0.2 */
    float critic_coef;              /* 5   */
    float bounds_coef;              /* 10  */
} DwaLoss;

int dwa_abi_version(void);
const char *dwa_last_error(void);

/* Bytes of device workspace dwa_act / dwa_critic (grad = 0) or dwa_grad (grad = 1) need for `rows` rows; -1 for bad arguments. */
int64_t dwa_workspace_bytes(int32_t rows, int32_t D, int32_t A, int32_t grad);
/* Bytes of device workspace dwa_stats needs. */
int64_t dwa_stats_workspace_bytes(int32_t D);

/* RunningMeanStd update: stats_out = combine(stats_in, batch mean / unbiased var / count of x [B][D]).  stats_out may equal stats_in. */
int dwa_stats(const float *x, int32_t B, int32_t D, const double *stats_in, double *stats_out, void *work, void *stream);

/* Eval-mode rollout step over N rows: obs [N][D], noise [N][A] (standard normal draws), logstd [A] ->
 * action [N][A] = mu + exp(logstd) noise, clamped [N][A] = clamp(action, -1, 1), mu [N][A], neglogp [N] of action, value [N] unnormalised
 * with stats_val.  obs_stats and val_stats stay. */
int dwa_act(const float *p, const double *obs_stats, const double *val_stats, const float *logstd, const float *obs, const float *noise,
            int32_t N, int32_t D, int32_t A, float *action, float *clamped, float *mu, float *neglogp, float *value, void *work, int64_t work_bytes,
            void *stream);

/* Bootstrap values: value [N] = unnorm(critic(obs)) * (1 - terminate [N]). */
int dwa_critic(const float *p, const double *obs_stats, const double *val_stats, const float *obs, const float *terminate, int32_t N, int32_t D,
               int32_t A, float *value, void *work, int64_t work_bytes, void *stream);

/* g += d(a_loss + critic_coef c_loss + bounds_coef b_loss)/dp for one minibatch of B rows: obs [B][D] normalised with obs_stats (the snapshot
 * the minibatch's dwa_stats left), act [B][A], old_nlp [B], adv [B], ret_n [B] (the normalised returns); the losses are added to state. */
int dwa_grad(const float *p, const double *obs_stats, const float *logstd, const float *obs, const float *act, const float *old_nlp,
             const float *adv, const float *ret_n, int32_t B, int32_t D, int32_t A, DwaLoss coef, float *g, float *state, void *work,
             int64_t work_bytes, void *stream);

/* Adam step of p with g (lr = state[DWA_S_LR], step count state[DWA_S_STEP] advanced on the device), then g = 0. */
int dwa_opt(float *p, float *g, float *m, float *v, float *state, int32_t D, int32_t A, void *stream);

/* GAE over a horizon of H steps of N envs ([H][N] each): adv = discount_values(done, values, rewards, next_values), ret = adv + values.
 * gamma_tau is the product gamma * tau as the reference forms it (in double, then used as an fp32 scalar). */
int dwa_gae(const float *done, const float *values, const float *rewards, const float *next_values, int32_t H, int32_t N, float gamma,
            float gamma_tau, float *adv, float *ret, void *stream);

/* Bytes of device workspace dwa_play needs for N rows (0: none, work may be NULL); -1 for bad arguments. */
int64_t dwa_play_workspace_bytes(int32_t N, int32_t D, int32_t A);

/* Play-time policy over N rows, the actor only: x = clamp((obs - mean) / sqrt(var + 1e-5), -5, 5) with obs_stats (eval mode: they stay),
 * mu [N][A] = W3 relu(W2 relu(W1 x + b1) + b2) + b3; clamped [N][A] = clamp(mu, -1, 1) with noise == NULL (the deterministic player), else
 * clamp(mu + exp(logstd) noise, -1, 1) with noise [N][A] standard normal draws (logstd may be NULL without noise).  mu may be NULL.
 * N <= 64 runs three launches of column slices (work: dwa_play_workspace_bytes), larger N one launch of 16-row workgroups. */
int dwa_play(const float *p, const double *obs_stats, const float *logstd, const float *obs, const float *noise, int32_t N, int32_t D, int32_t A,
             float *clamped, float *mu, void *work, int64_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
