// dw_amp_stats.h -- the per-env update and the reduction of TocabiAMPLower's episode statistics (include/dyros_amp_stats.h), written once for
// the HIP kernels of dw_amp_stats.hip and for a g++ build (tests/amp_stats_host.cpp), which the CPU tests hold against a numpy restatement.
// The termination predicates restate dwa::reset (dw_amp.h) and the fused step's termination role (dw_amp_step.h) term by term.
#ifndef DW_AMP_STATS_H
#define DW_AMP_STATS_H

#include <math.h>
#include <stdint.h>

#include "dw_amp.h"
#include "../../include/dyros_amp_stats.h"
#include "dw_episode.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace dwe {

constexpr int NB = DWE_BODIES;
static_assert(NB == DW_NUM_BODIES, "contact_forces / rigid_body_pos rows");

using epi::f2u;
using epi::partial;
using epi::Rows;
using epi::RT;
using epi::u2f;

// a component over 1 (the step tests components, not the norm)
struct Over1 {
    EPI_HD bool operator()(float x, float y, float z) const { return x > 1.0f || y > 1.0f || z > 1.0f; }
};

// bit g of (lo | hi << 32): Gym body g (not a sole) has a component over 1
DW_HD void contact_mask(const float *cf, uint32_t &lo, uint32_t &hi) { epi::contact_mask<NB, DWE_LFOOT, DWE_RFOOT>(cf, lo, hi, Over1{}); }

struct Cfg {
    float max_len, term_h, cmd_lo, cmd_hi;
    int eet;
};

// one env's words of the step's buffers
struct EnvIn {
    const float *root;        // [13] root_states row
    const float *rv;          // [9]  reward_values row
    const float *cmd;         // [3]  commands row
    float fzl, fzr;           // contact_forces[8 / 16][2]
    float zl, zr;             // rigid_body_pos[8 / 16][2]
    float rew, total_mass;
    int p, reset;
};

// the running episode of one env (the DWE_ST_* words) and the window sums every record adds to, held in registers between one load and one
// store: every global load of an update is issued before the first store
struct St {
    int n, prev, closed;
    float ret, pkl, pkr;
};
struct AcHot {
    float rew[DWE_REW_TERMS], verr[DWE_CMD_BINS], vcnt[DWE_CMD_BINS], yaw;
};

DW_HD St load(const Rows &r) {
    St s;
    s.n = (int)r.w(DWE_ST_N); s.prev = (int)r.w(DWE_ST_PREV); s.closed = (int)r.w(DWE_ST_CLOSED);
    s.ret = u2f(r.w(DWE_ST_RET)); s.pkl = u2f(r.w(DWE_ST_PKL)); s.pkr = u2f(r.w(DWE_ST_PKR));
    return s;
}
DW_HD void store(const Rows &r, const St &s) {
    r.w(DWE_ST_N) = (uint32_t)s.n; r.w(DWE_ST_PREV) = (uint32_t)s.prev; r.w(DWE_ST_CLOSED) = (uint32_t)s.closed;
    r.w(DWE_ST_RET) = f2u(s.ret); r.w(DWE_ST_PKL) = f2u(s.pkl); r.w(DWE_ST_PKR) = f2u(s.pkr);
}
DW_HD AcHot load_hot(const Rows &r) {
    AcHot h;
    for (int k = 0; k < DWE_REW_TERMS; ++k) h.rew[k] = r.a(DWE_AC_REW + k);
    for (int k = 0; k < DWE_CMD_BINS; ++k) { h.verr[k] = r.a(DWE_AC_VERR + k); h.vcnt[k] = r.a(DWE_AC_VCNT + k); }
    h.yaw = r.a(DWE_AC_YAW);
    return h;
}
// bin: the command bin this record added to, -1: the record added no sample (nothing to store)
DW_HD void store_hot(const Rows &r, const AcHot &h, int bin) {
    if (bin < 0) return;
    for (int k = 0; k < DWE_REW_TERMS; ++k) r.a(DWE_AC_REW + k) = h.rew[k];
    for (int k = 0; k < DWE_CMD_BINS; ++k)
        if (k == bin) { r.a(DWE_AC_VERR + k) = h.verr[k]; r.a(DWE_AC_VCNT + k) = h.vcnt[k]; }
    r.a(DWE_AC_YAW) = h.yaw;
}

// 4 equal bins over [lo, hi]; anything outside (or not a number) goes to the nearest end
DW_HD int cmd_bin(float c, float lo, float hi) {
    const float u = (c - lo) / (hi - lo) * (float)DWE_CMD_BINS;
    if (!(u >= 0.0f)) return 0;
    if (u >= (float)DWE_CMD_BINS) return DWE_CMD_BINS - 1;
    return (int)u;
}

// the step's termination test (tasks/amp/tocabi_amp_lower_base.py:1025-1069), one bit per term; any: a non-sole body has a component over 1
DW_HD int cause_mask(const EnvIn &in, bool any_contact, const Cfg &C) {
    int m = ((float)in.p >= C.max_len - 1.0f) ? DWE_C_TIME : 0;
    if (C.eet && in.p > 1) {
        if (any_contact) m |= DWE_C_CONTACT;
        if (in.root[2] < C.term_h) m |= DWE_C_LOW;
        if (in.zl > 0.5f || in.zr > 0.5f) m |= DWE_C_FLY;
        const float q0[4] = {in.root[3], in.root[4], in.root[5], in.root[6]};
        if (fabsf(dw::quat_err(q0)) > (float)(3.141592 / 4.0)) m |= DWE_C_TILT;
    }
    return m;
}

// One env after one step, on its state s and hot sums h (the caller loads and stores them); the sums of an ended episode go to r.  C: add(word, v)
// and max(word, v) on the integer counts.  Returns the cause mask; bin: see store_hot.
template <class CT>
DW_HD int update(const EnvIn &in, uint32_t mlo, uint32_t mhi, St &s, AcHot &h, const Rows &r, CT &c, const Cfg &C, int &bin) {
    const int mask = cause_mask(in, (mlo | mhi) != 0u, C);
    const int p = in.p;
    bin = -1;
    const bool next = p == s.prev + 1;
    if (s.closed && s.n >= 0 && next) {                   // 1. an ended env the caller did not reset
        c.add(DWE_CT_UNRESET, 1);
        s.prev = p;
        return mask;
    }
    if (s.closed || s.n < 0 || !next) {                   // 2. a new episode starts with this step
        if (s.n >= 0 && !s.closed) c.add(DWE_CT_DISCARDED, 1);
        s.n = 0;
        s.closed = 0;
        s.ret = s.pkl = s.pkr = 0.0f;
    }
    s.prev = p;
    s.n += 1;                                             // 3. this step's samples
    bool finite = true;
    for (int k = 0; k < 13; ++k) finite = finite && dw::finitef(in.root[k]);
    if (!finite) {
        c.add(DWE_CT_NONFINITE, 1);
    } else {
        c.add(DWE_CT_SAMPLES, 1);
        s.ret = s.ret + in.rew;
        for (int k = 0; k < DWE_REW_TERMS; ++k) h.rew[k] = h.rew[k] + in.rv[k];
        const float q[4] = {in.root[3], in.root[4], in.root[5], in.root[6]}, v[3] = {in.root[7], in.root[8], in.root[9]};
        float lv[3];
        dwa::quat_rotate_inverse(q, v, lv);
        bin = cmd_bin(in.cmd[0], C.cmd_lo, C.cmd_hi);
        const float ev = fabsf(in.cmd[0] - lv[0]);
        for (int k = 0; k < DWE_CMD_BINS; ++k)
            if (k == bin) { h.verr[k] = h.verr[k] + ev; h.vcnt[k] = h.vcnt[k] + 1.0f; }
        h.yaw = h.yaw + fabsf(in.cmd[2] - in.root[12]);
        const float w = 9.81f * in.total_mass;
        s.pkl = fmaxf(s.pkl, in.fzl / w);
        s.pkr = fmaxf(s.pkr, in.fzr / w);
        const float thr = (float)(1.4 * 9.81) * in.total_mass;          // (the reward's threshold, dwa::reward_row)
        if (in.fzl > thr) c.add(DWE_CT_SOLE_OVER, 1);
        if (in.fzr > thr) c.add(DWE_CT_SOLE_OVER + 1, 1);
    }
    if (in.reset) {                                       // 4. the episode ends with this step
        s.closed = 1;
        c.add(DWE_CT_EPISODES, 1);
        c.add(DWE_CT_MASK + mask, 1);
        c.add(DWE_CT_LEN_SUM, (uint32_t)p);
        c.max(DWE_CT_LEN_MAX, (uint32_t)p);
        const float u = (float)p * (float)DWE_LEN_BINS / C.max_len;
        const int hb = !(u >= 0.0f) ? 0 : (u >= (float)DWE_LEN_BINS ? DWE_LEN_BINS - 1 : (int)u);
        c.add(DWE_CT_LEN_HIST + hb, 1);
        if (mask & DWE_C_CONTACT)
            for (int g = 0; g < NB; ++g)
                if (((g < 32 ? mlo >> g : mhi >> (g - 32)) & 1u) != 0u) c.add(DWE_CT_BODY + g, 1);
        r.a(DWE_AC_RET) += s.ret;
        r.a(DWE_AC_PK) += s.pkl;
        r.a(DWE_AC_PK + 1) += s.pkr;
    }
    return mask;
}

// once per record
DW_HD void count_call(uint64_t *ct) {
    ct[DWE_CT_CALLS] += 1;
    ct[DWE_CT_RECORDS] += 1;
}

}  // namespace dwe

#endif
