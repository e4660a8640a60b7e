// dw_stats.h -- the per-env update and the reduction of the episode statistics (include/dyros_stats.h), written once for the HIP kernels
// of dw_stats.hip and for a g++ build (tests/stats_host.cpp), which the CPU tests hold against a numpy restatement.
#ifndef DW_STATS_H
#define DW_STATS_H

#include <math.h>
#include <stdint.h>

#include "../../include/dyros_walk.h"
#include "../../include/dyros_stats.h"
#include "dw_episode.h"

#if defined(__HIPCC__)
#define DWS_HD __host__ __device__ inline
#else
#define DWS_HD inline
#endif

namespace dws {

constexpr int NB = DW_NUM_BODIES, ESW = DW_ES_WORDS;

using epi::f2u;
using epi::partial;
using epi::Rows;
using epi::RT;
using epi::u2f;

// |F| > 1 N exactly as the step kernel's collision test forms it (dw_limb.h over_1n: torch.norm's order for three elements)
struct Over1N {
    DWS_HD bool operator()(float x, float y, float z) const {
        float b = fmaf(x, x, 0.0f);
        b = fmaf(y, y, b);
        b = fmaf(z, z, b);
        return sqrtf(b) > 1.0f;
    }
};

// bit g of (lo | hi << 32): Gym body g (not a sole) is over 1 N
DWS_HD void contact_mask(const float *cf, uint32_t &lo, uint32_t &hi) { epi::contact_mask<NB, DWS_LFOOT, DWS_RFOOT>(cf, lo, hi, Over1N{}); }

// one env's words of the step's buffers
struct EnvIn {
    const float *cf;          // [38 * 3] contact_forces row
    const float *root;        // [13]     root_states row
    const float *tq;          // [12]     action_torque
    float tv0, tv1, tf0, tf1, last_return, total_mass;
    int pert_on, nan_resets, reset;
};

// the running episode of one env (the DWS_ST_* words), held in registers between one load and one store: every global load of an update is
// issued before the first store, so a record is one memory round trip deep
struct St {
    int n, nan, nr, pert, off;
    float x0, y0, xl, yl, tv0, verr, pkl, pkr, dtm;
    float tau[12];
};

DWS_HD St load(const Rows &r) {
    St s;
    s.n = (int)r.w(DWS_ST_N); s.nan = (int)r.w(DWS_ST_NAN); s.nr = (int)r.w(DWS_ST_NR); s.pert = (int)r.w(DWS_ST_PERT); s.off = (int)r.w(DWS_ST_OFF);
    s.x0 = u2f(r.w(DWS_ST_X0)); s.y0 = u2f(r.w(DWS_ST_Y0)); s.xl = u2f(r.w(DWS_ST_XL)); s.yl = u2f(r.w(DWS_ST_YL)); s.tv0 = u2f(r.w(DWS_ST_TV0));
    s.verr = u2f(r.w(DWS_ST_VERR)); s.pkl = u2f(r.w(DWS_ST_PKL)); s.pkr = u2f(r.w(DWS_ST_PKR)); s.dtm = u2f(r.w(DWS_ST_DTM));
    for (int j = 0; j < 12; ++j) s.tau[j] = u2f(r.w(DWS_ST_TAU + j));
    return s;
}

DWS_HD void store(const Rows &r, const St &s) {
    r.w(DWS_ST_N) = (uint32_t)s.n; r.w(DWS_ST_NAN) = (uint32_t)s.nan; r.w(DWS_ST_NR) = (uint32_t)s.nr; r.w(DWS_ST_PERT) = (uint32_t)s.pert;
    r.w(DWS_ST_OFF) = (uint32_t)s.off;
    r.w(DWS_ST_X0) = f2u(s.x0); r.w(DWS_ST_Y0) = f2u(s.y0); r.w(DWS_ST_XL) = f2u(s.xl); r.w(DWS_ST_YL) = f2u(s.yl); r.w(DWS_ST_TV0) = f2u(s.tv0);
    r.w(DWS_ST_VERR) = f2u(s.verr); r.w(DWS_ST_PKL) = f2u(s.pkl); r.w(DWS_ST_PKR) = f2u(s.pkr); r.w(DWS_ST_DTM) = f2u(s.dtm);
    for (int j = 0; j < 12; ++j) r.w(DWS_ST_TAU + j) = f2u(s.tau[j]);
}

// the window sums every record adds to (the others only change when an episode ends)
struct AcHot {
    float ft0, ft1, tau;
};

DWS_HD AcHot load_hot(const Rows &r) { return AcHot{r.a(DWS_AC_FT), r.a(DWS_AC_FT + 1), r.a(DWS_AC_TAU)}; }
DWS_HD void store_hot(const Rows &r, const AcHot &h) { r.a(DWS_AC_FT) = h.ft0; r.a(DWS_AC_FT + 1) = h.ft1; r.a(DWS_AC_TAU) = h.tau; }

// a new episode's counters: after an in-step reset (steps = 0) or on an explicit restart (steps = progress_buf)
DWS_HD void begin(St &s, int steps, const float *root, float tv0, int pert_on, int nan_resets) {
    s.n = steps;
    s.nan = nan_resets;
    s.nr = 0;
    s.pert = pert_on;
    s.off = pert_on ? 0 : DWS_OFF_NEVER;
    s.x0 = s.xl = root[0];
    s.y0 = s.yl = root[1];
    s.tv0 = tv0;
    s.verr = s.pkl = s.pkr = s.dtm = 0.0f;
    for (int j = 0; j < 12; ++j) s.tau[j] = 0.0f;
}

DWS_HD int cmd_bin(float tv0) {
    int b = (int)(tv0 / 0.2f);
    return b < 0 ? 0 : (b > DWS_CMD_BINS - 1 ? DWS_CMD_BINS - 1 : b);
}

// One env after one step, on its state s and hot sums h (the caller loads and stores them); the sums of an ended episode go to r.  C: add(word, v)
// and max(word, v) on the integer counts.  Returns the cause code.
// Terminal-step rule: root_states, target_vel and pert_on are the NEW episode's after an in-step reset, so they are skipped on that step;
// contact_forces and action_torque are the terminal step's and count.
// Torque difference: the step kernel has already copied this step's action_torque into action_torque_pre when a record runs (its late update,
// the reference's post_physics_step), so the previous record's action_torque is kept in s.tau.  The first record of an episode (s.nr == 0: no
// earlier record of the same episode) has no previous torque of its own and adds no difference.
template <class C>
DWS_HD int update(const EnvIn &in, uint32_t mlo, uint32_t mhi, St &s, AcHot &h, const Rows &r, C &c, float max_len, float dt_policy) {
    const float fl = in.cf[3 * DWS_LFOOT + 2], fr = in.cf[3 * DWS_RFOOT + 2];
    const float pkl = fmaxf(s.pkl, fl), pkr = fmaxf(s.pkr, fr);
    const float ws = in.total_mass / 104.48f;
    h.ft0 += fabsf(fl + ws * in.tf0);
    h.ft1 += fabsf(fr + ws * in.tf1);
    float tau = 0.0f;
    for (int j = 0; j < 12; ++j) tau += fabsf(in.tq[j]);
    h.tau += tau;
    if (s.nr > 0) {
        float dtm = s.dtm;
        for (int j = 0; j < 12; ++j) dtm = fmaxf(dtm, fabsf(in.tq[j] - s.tau[j]));
        s.dtm = dtm;
    }
    const int n = s.n + 1;
    if (!in.reset) {
        for (int j = 0; j < 12; ++j) s.tau[j] = in.tq[j];
        const float dx = in.tv0 - in.root[7], dy = in.tv1 - in.root[8];
        s.verr = s.verr + sqrtf(dx * dx + dy * dy);
        s.nr += 1;
        s.xl = in.root[0];
        s.yl = in.root[1];
        if (in.pert_on) {
            if (!s.pert) c.add(DWS_CT_PUSHES, 1);
            s.off = 0;
        } else {
            s.off = s.off >= DWS_OFF_NEVER ? DWS_OFF_NEVER : s.off + 1;
        }
        s.pert = in.pert_on ? 1 : 0;
        s.n = n;
        s.nan = in.nan_resets;
        s.pkl = pkl;
        s.pkr = pkr;
        return DWS_CAUSE_NONE;
    }
    const int cause = in.nan_resets > s.nan ? DWS_CAUSE_NON_FINITE
                    : (mlo | mhi) != 0u ? DWS_CAUSE_NON_FOOT_CONTACT
                    : (float)n >= max_len - 1.0f ? DWS_CAUSE_TIME_LIMIT : DWS_CAUSE_ORIENTATION;
    c.add(DWS_CT_EPISODES, 1);
    c.add(DWS_CT_CAUSE + cause, 1);
    c.add(DWS_CT_LEN_SUM, (uint32_t)n);
    c.max(DWS_CT_LEN_MAX, (uint32_t)n);
    int hb = (int)((float)n * (float)DWS_LEN_BINS / max_len);
    hb = hb < 0 ? 0 : (hb > DWS_LEN_BINS - 1 ? DWS_LEN_BINS - 1 : hb);
    c.add(DWS_CT_LEN_HIST + hb, 1);
    if (cause == DWS_CAUSE_NON_FOOT_CONTACT)
        for (int g = 0; g < NB; ++g)
            if (((g < 32 ? mlo >> g : mhi >> (g - 32)) & 1u) != 0u) c.add(DWS_CT_BODY + g, 1);
    r.a(DWS_AC_RET) += in.last_return;
    const int b = cmd_bin(s.tv0);
    c.add(DWS_CT_BIN_EP + b, 1);
    if (s.nr > 0) {
        c.add(DWS_CT_BIN_ROOT + b, 1);
        r.a(DWS_AC_VERR + b) += s.verr / (float)s.nr;
        r.a(DWS_AC_DRIFT + b) += fabsf(s.yl - s.y0);
        const float dist = s.tv0 * ((float)s.nr * dt_policy);
        if (dist >= DWS_RATIO_MIN_M) {
            c.add(DWS_CT_BIN_RATIO + b, 1);
            r.a(DWS_AC_RATIO + b) += (s.xl - s.x0) / dist;
        }
    }
    r.a(DWS_AC_PK) += pkl;
    r.a(DWS_AC_PK + 1) += pkr;
    if (pkl > DWS_SOLE_LIMIT) c.add(DWS_CT_PK_OVER, 1);
    if (pkr > DWS_SOLE_LIMIT) c.add(DWS_CT_PK_OVER + 1, 1);
    r.a(DWS_AC_DTM) += s.dtm;
    if (cause != DWS_CAUSE_TIME_LIMIT && s.off + 1 <= DWS_PUSH_WINDOW) c.add(DWS_CT_PUSH_FALLS, 1);
    begin(s, 0, in.root, in.tv0, in.pert_on, in.nan_resets);
    return cause;
}

// the gate of the perturbations (tasks/dyros_dynamic_walk.py:492 tests env 0) and the record counts: once per record
DWS_HD void count_call(uint64_t *ct, int env0_perturb_start) {
    const uint64_t call = ct[DWS_CT_CALLS];
    if (env0_perturb_start && ct[DWS_CT_GATE_AT] == 0) ct[DWS_CT_GATE_AT] = call + 1;
    ct[DWS_CT_CALLS] = call + 1;
    ct[DWS_CT_RECORDS] += 1;
}

}  // namespace dws

#endif
