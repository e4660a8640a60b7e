/* dyros_amp_disc.h -- C-ABI of the on-GPU AMP discriminator (the consumer's side of TocabiAMPLower).
 *
 * What it replaces (reference: learning/amp_continuous.py, learning/amp_network_builder.py:74-110, cfg/train/TocabiAMPLowerPPO.yaml):
 *   dwd_reward  _calc_disc_rewards + _combine_rewards (:505-532) with the eval-mode _preproc_amp_obs: ONE launch
 *   dwd_stats   the train-mode update of rl_games' RunningMeanStd inside _preproc_amp_obs (:500-503)
 *   dwd_grad    the discriminator's share of calc_gradients (:273-329): forward of the agent, replay and demo rows, _disc_loss
 *               (:404-457) with the gradient penalty as an analytic double backward, times disc_coef, backward to every parameter
 *   dwd_opt     the optimiser step of those parameters (torch.optim.Adam, betas 0.9 / 0.999, eps 1e-8, no clipping)
 * The network: x [D] -> relu(W1 x + b1) [256] -> relu(W2 h1 + b2) [256] -> w3 . h2 + b3 (the logit); fp32 throughout.
 * All pointers are device pointers; every function enqueues on `stream` and returns 0, or -1 with dwd_last_error() set.  No function
 * reads anything but its arguments, so every launch can be captured in a graph and replayed.
 *
 * Parameter layout (fp32, `p`; the gradient `g`, Adam moments `m`, `v` have the same layout), D = num_amp_obs:
 *   W1 [HID][D] | b1 [HID] | W2 [HID][HID] | b2 [HID] | w3 [HID] | b3 [1]           (DWD_NP(D) floats; W rows = outputs, as nn.Linear)
 * Running statistics (`stats`, fp64 as rl_games keeps them): mean [D] | var [D] | count [1]       (DWD_NSTATS(D) doubles)
 * D is any multiple of DWD_OBS_STEP up to DWD_D_MAX; tiles pad it with zeros internally. */
#ifndef DYROS_AMP_DISC_H
#define DYROS_AMP_DISC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWD_ABI_VERSION 1
#define DWD_HID       256   /* cfg/train/TocabiAMPLowerPPO.yaml network.disc.units [256, 256]: the only width accepted */
#define DWD_OBS_STEP  34    /* AMP observation words per step (tocabi_amp_lower.py NUM_AMP_OBS_PER_STEP) */
#define DWD_D_MAX     340   /* numAMPObsSteps <= 10 */
#define DWD_NP(D)     ((D) * DWD_HID + DWD_HID + DWD_HID * DWD_HID + DWD_HID + DWD_HID + 1)
#define DWD_NSTATS(D) (2 * (D) + 1)

/* float words of `state` (device memory, zeroed by the caller): dwd_grad ADDS one minibatch's values, the caller divides by S_UPDATES */
#define DWD_S_LOSS        0   /* disc_coef * disc_loss                                                        */
#define DWD_S_PRED        1   /* 0.5 * (BCE(agent + replay logits, 0) + BCE(demo logits, 1))                 */
#define DWD_S_LOGIT_REG   2   /* sum of the logit weights squared (disc_logit_loss)                           */
#define DWD_S_GRAD_PEN    3   /* mean over the demo rows of |d logit / d x_demo|^2 (disc_grad_penalty)         */
#define DWD_S_WEIGHT_DEC  4   /* sum of every weight squared                                                 */
#define DWD_S_AGENT_LOGIT 5   /* mean logit of the agent + replay rows                                        */
#define DWD_S_DEMO_LOGIT  6   /* mean logit of the demo rows                                                  */
#define DWD_S_AGENT_ACC   7   /* fraction of agent + replay logits < 0 (_compute_disc_acc)                    */
#define DWD_S_DEMO_ACC    8   /* fraction of demo logits > 0                                                  */
#define DWD_S_UPDATES     9   /* minibatches accumulated                                                      */
#define DWD_S_LR          12  /* Adam: learning rate (the caller's schedule writes it)                        */
#define DWD_S_STEP        13  /* Adam: steps taken                                                            */
#define DWD_S_WORDS       16

typedef struct DwdLoss {            /* the yaml's coefficients */
    float disc_coef;                /* 5      */
    float logit_reg;                /* 0.05   */
    float grad_penalty;             /* 0.1    */
    float weight_decay;             /* 1e-4   */
} DwdLoss;

int dwd_abi_version(void);
const char *dwd_last_error(void);

/* Bytes of device workspace dwd_grad needs for these row counts (dwd_reward needs none beyond its arguments). */
int64_t dwd_grad_workspace_bytes(int32_t D, int32_t n_agent, int32_t n_replay, int32_t n_demo);
/* Bytes of device workspace dwd_stats needs. */
int64_t dwd_stats_workspace_bytes(int32_t D);

/* amp_obs [B][D] -> logits [B] (or NULL), disc_r [B] = -log(max(1 - sigmoid(logit), 1e-4)) * reward_scale,
 * combined [B] = task_w * task_rew[B] + disc_w * disc_r, with the statistics `stats` fixed (eval mode). ONE launch. */
int dwd_reward(const float *p, const double *stats, const float *amp_obs, const float *task_rew, int32_t B, int32_t D, float reward_scale,
               float task_w, float disc_w, float *disc_r, float *combined, float *logits, void *stream);

/* RunningMeanStd update: stats_out = combine(stats_in, batch mean / unbiased var / count of x [B][D]).  stats_out may equal stats_in. */
int dwd_stats(const float *x, int32_t B, int32_t D, const double *stats_in, double *stats_out, void *work, void *stream);

/* g += d(disc_coef * disc_loss)/dp for one minibatch: agent [n_agent][D] normalised with stats_agent, replay [n_replay][D] with stats_replay,
 * demo [n_demo][D] with stats_demo (the three successive snapshots train mode leaves); the loss terms are added to state. */
int dwd_grad(const float *p, const float *agent, int32_t n_agent, const float *replay, int32_t n_replay, const float *demo, int32_t n_demo, int32_t D,
             const double *stats_agent, const double *stats_replay, const double *stats_demo, DwdLoss coef, float *g, float *state, void *work,
             int64_t work_bytes, void *stream);

/* Adam step of p with g (lr = state[DWD_S_LR], step count state[DWD_S_STEP] advanced on the device), then g = 0. */
int dwd_opt(float *p, float *g, float *m, float *v, float *state, int32_t D, void *stream);

#ifdef __cplusplus
}
#endif

#endif
