// dw_gait.h -- one env's sample of the gait profile (include/dyros_gait.h), written once for the HIP kernels of dw_gait.hip and for a g++
// build (tests/gait_host.cpp), which the CPU tests hold against a numpy restatement.
#ifndef DW_GAIT_H
#define DW_GAIT_H

#include <math.h>
#include <stdint.h>

#include "../../include/dyros_walk.h"
#include "../../include/dyros_stats.h"
#include "../../include/dyros_gait.h"

#if defined(__HIPCC__)
#define DWG_HD __host__ __device__ inline
#else
#define DWG_HD inline
#endif

namespace dwg {

constexpr int W = DWG_W, NJ = DWG_LEG_JOINTS, ESW = DW_ES_WORDS;
enum Class { RECORDED = DWG_CT_RECORDED, TERMINAL = DWG_CT_SKIPPED_TERMINAL, FILTERED = DWG_CT_SKIPPED_FILTER, DISCARDED = DWG_CT_DISCARDED };

DWG_HD bool bins_ok(int b) { return b == 12 || b == 24 || b == 36 || b == 72 || b == 144; }
DWG_HD int groups(int n) { return (n + DWG_GROUP - 1) / DWG_GROUP; }

// the reward's window of mocap row idx (dw_oct_post.h: DSP, RSSP, LSSP)
DWG_HD int window_of(int idx) {
    if (300 <= idx && idx < 1500) return DWG_WIN_RSSP;
    if (2100 <= idx && idx < 3300) return DWG_WIN_LSSP;
    return DWG_WIN_DSP;
}

// the fixed-point image of a sample: 2^-16 units, round to nearest even, |v| clamped to 2^30 first (v is finite)
DWG_HD int64_t fx(double v) {
    const double lim = (double)(1 << DWG_CLAMP_LOG2);
    v = v > lim ? lim : (v < -lim ? -lim : v);
    return (int64_t)llrint(v * (double)(1 << DWG_FRAC_BITS));
}

// one env's words of the step's buffers
struct EnvIn {
    float fl, fr;                   // F_z of the soles
    float total_mass, tf0, tf1;     // target_data_force
    float root_z, root_vx, tv0;
    float paid;                     // stacked_rewards[DWG_PAID_COLUMN]
    const float *dof_pos;           // [12] at stride dof_stride
    int dof_stride;
    const float *tq;                // [12] action_torque
    const float *tqpos;             // [12] target_data_qpos
    int mocap_idx, pert_on, reset;
    int64_t progress;
};

DWG_HD bool fin(float x) { return isfinite(x); }

// The class of one env-step; a RECORDED one adds the DWG_W words of its row to bin b through A: a.bin(b) once, then a.add(b, word, addend)
// for every word (the adder may drop zero addends).
template <class A>
DWG_HD int sample(const EnvIn &in, int bins, int min_episode_step, int skip_pushes, const A &a) {
    if (in.reset) return TERMINAL;
    if (in.progress < (int64_t)min_episode_step || (skip_pushes && in.pert_on)) return FILTERED;
    bool ok = fin(in.fl) && fin(in.fr) && fin(in.total_mass) && fin(in.tf0) && fin(in.tf1) && fin(in.root_z) && fin(in.root_vx) && fin(in.tv0) &&
              fin(in.paid) && in.mocap_idx >= 0 && in.mocap_idx < DWG_ROWS;
    for (int j = 0; j < NJ; ++j) ok = ok && fin(in.dof_pos[j * in.dof_stride]) && fin(in.tq[j]) && fin(in.tqpos[j]);
    if (!ok) return DISCARDED;
    const int width = DWG_ROWS / bins;
    const int b = in.mocap_idx / width;
    const float ws = in.total_mass / 104.48f;
    const bool lcon = in.fl > 1.0f, rcon = in.fr > 1.0f;
    const int win = window_of(b * width);
    const bool pay = win == DWG_WIN_DSP ? (rcon && lcon) : (win == DWG_WIN_RSSP ? (rcon && !lcon) : (!rcon && lcon));
    a.bin(b);
    a.add(b, DWG_R_COUNT, 1);
    a.add(b, DWG_R_FZ, fx((double)in.fl));
    a.add(b, DWG_R_FZ + 1, fx((double)in.fr));
    a.add(b, DWG_R_FZ2, fx((double)in.fl * (double)in.fl));
    a.add(b, DWG_R_FZ2 + 1, fx((double)in.fr * (double)in.fr));
    a.add(b, DWG_R_EXPECTED, fx((double)(-(ws * in.tf0))));
    a.add(b, DWG_R_EXPECTED + 1, fx((double)(-(ws * in.tf1))));
    a.add(b, DWG_R_FERR, fx((double)fabsf(in.fl + ws * in.tf0)));
    a.add(b, DWG_R_FERR + 1, fx((double)fabsf(in.fr + ws * in.tf1)));
    a.add(b, DWG_R_CONTACT, lcon ? 1 : 0);
    a.add(b, DWG_R_CONTACT + 1, rcon ? 1 : 0);
    a.add(b, DWG_R_PAID, in.paid > 0.0f ? 1 : 0);
    a.add(b, DWG_R_PREDICTED, pay ? 1 : 0);
    a.add(b, DWG_R_ROOT_Z, fx((double)in.root_z));
    a.add(b, DWG_R_VEL_ERR, fx((double)(in.root_vx - in.tv0)));
    a.add(b, DWG_R_PERT, in.pert_on ? 1 : 0);
    for (int j = 0; j < NJ; ++j) {
        a.add(b, DWG_R_JOINT_ERR + j, fx((double)fabsf(in.dof_pos[j * in.dof_stride] - in.tqpos[j])));
        a.add(b, DWG_R_TORQUE + j, fx((double)fabsf(in.tq[j])));
    }
    return RECORDED;
}

}  // namespace dwg

#endif
