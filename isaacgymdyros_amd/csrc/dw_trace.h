// dw_trace.h -- the row assembly and the slot state of the run trace (include/dyros_trace.h), written once for the HIP kernels of
// dw_trace.hip and for a g++ build (tests/trace_host.cpp), which the CPU tests hold against a numpy restatement.
#ifndef DW_TRACE_H
#define DW_TRACE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dyros_walk.h"
#include "../../include/dyros_stats.h"
#include "../../include/dyros_trace.h"
#include "dw_episode.h"

#if defined(__HIPCC__)
#define DWT_HD __host__ __device__ inline
#else
#define DWT_HD inline
#endif

namespace dwt {

constexpr int NB = DW_NUM_BODIES, ESW = DW_ES_WORDS, ROW = DWT_ROW_WORDS, CFW = DW_NUM_BODIES * 3;

using epi::f2u;
using epi::u2f;

// The source spans of a row's float words.  Word i of a span (0 <= i < len) comes from word src + i of the env's row of buffer `buf` and
// goes to row word dst_of(span, i): consecutive i are consecutive source words, and -- but for the de-interleave of dof_state --
// consecutive row words.  No span is longer than a wavefront, so a span is one load per lane.
enum Buf { B_ROOT, B_DOF, B_ES, B_STACKED, B_REW, B_COUNT };
struct Span {
    int buf, src, len, dst;
};
constexpr int NSPAN = 12;
constexpr int DOF_SPLIT = 64;          // dof_state's 66 interleaved words: one span of 64, one of 2
DWT_HD Span span(int k) {
    switch (k) {
    case 0: return Span{B_ROOT, 0, DWT_LEN_ROOT, DWT_CH_ROOT};
    case 1: return Span{B_DOF, 0, DOF_SPLIT, DWT_CH_DOF_POS};
    case 2: return Span{B_DOF, DOF_SPLIT, 2 * DW_NUM_DOF - DOF_SPLIT, DWT_CH_DOF_POS};
    case 3: return Span{B_ES, DW_ES_QPOS_NOISE, DWT_LEN_QPOS_NOISE, DWT_CH_QPOS_NOISE};
    case 4: return Span{B_ES, DW_ES_TARGET_QPOS, DWT_LEN_TARGET_QPOS, DWT_CH_TARGET_QPOS};
    case 5: return Span{B_ES, DW_ES_ACTIONS, DWT_LEN_ACTIONS, DWT_CH_ACTIONS};
    case 6: return Span{B_ES, DW_ES_ACTION_TORQUE, DWT_LEN_TORQUE, DWT_CH_TORQUE};
    case 7: return Span{B_ES, DW_ES_TARGET_FORCE, DWT_LEN_TARGET_FORCE + DWT_LEN_TARGET_VEL, DWT_CH_TARGET_FORCE};   // (adjacent in both)
    case 8: return Span{B_ES, DW_ES_MAGNITUDE, DWT_LEN_MAGNITUDE + DWT_LEN_PHASE, DWT_CH_MAGNITUDE};                  // (adjacent in both)
    case 9: return Span{B_ES, DW_ES_TIME, DWT_LEN_TIME, DWT_CH_TIME};
    case 10: return Span{B_STACKED, 0, DWT_LEN_STACKED, DWT_CH_STACKED};
    default: return Span{B_REW, 0, DWT_LEN_REW, DWT_CH_REW};          // (k == 11: the one word of rew_buf)
    }
}
static_assert(DW_ES_TARGET_VEL == DW_ES_TARGET_FORCE + 2 && DWT_CH_TARGET_VEL == DWT_CH_TARGET_FORCE + 2, "target force and vel travel as one span");
static_assert(DW_ES_PHASE == DW_ES_MAGNITUDE + 1 && DWT_CH_PHASE == DWT_CH_MAGNITUDE + 1, "magnitude and phase travel as one span");
static_assert(DWT_LEN_DOF_POS == DW_NUM_DOF && DWT_LEN_DOF_VEL == DW_NUM_DOF && DWT_LEN_STACKED == DW_NUM_REW, "row lengths");
static_assert(DWT_CH_PAD + DWT_LEN_PAD == DWT_ROW_WORDS && DWT_ROW_WORDS % 4 == 0, "rows are whole 16-byte pieces");

DWT_HD int dst_of(const Span &s, int i) {
    if (s.buf != B_DOF) return s.dst + i;
    const int w = s.src + i;          // dof_state word 2 j + c: position (c = 0) or velocity (c = 1) of joint j
    return ((w & 1) ? DWT_CH_DOF_VEL : DWT_CH_DOF_POS) + (w >> 1);
}

// the per-env rows of the step's buffers
struct Src {
    const float *p[B_COUNT];
};
DWT_HD Src rows_of(int e, const float *root_states, const float *dof_state, const float *env_state, const float *rew_buf,
                   const float *stacked_rewards) {
    Src s;
    s.p[B_ROOT] = root_states + (size_t)e * 13;
    s.p[B_DOF] = dof_state + (size_t)e * 2 * DW_NUM_DOF;
    s.p[B_ES] = env_state + (size_t)e * ESW;
    s.p[B_STACKED] = stacked_rewards + (size_t)e * DW_NUM_REW;
    s.p[B_REW] = rew_buf + e;
    return s;
}

// |F| as the step kernel's collision test forms it (dws::over_1n: torch.norm's order for three elements)
DWT_HD float norm3(float x, float y, float z) {
    float b = fmaf(x, x, 0.0f);
    b = fmaf(y, y, b);
    b = fmaf(z, z, b);
    return sqrtf(b);
}

// The non-foot maximum.  Candidates are ordered by the bits of |F| without the sign: a total order on what a norm can be (non-negative
// numbers below infinity below NaNs), so a reduction gives the same winner in any association; among equals the lowest row wins.
struct Cand {
    uint32_t key;          // bits of |F| & 0x7fffffff
    int g;                 // Gym row; NB: no candidate
    float v;
};
DWT_HD Cand no_cand() { return Cand{0u, NB, 0.0f}; }
DWT_HD Cand cand_of(const float *cf, int g) {
    if (g >= NB || g == DWS_LFOOT || g == DWS_RFOOT) return no_cand();
    const float v = norm3(cf[3 * g], cf[3 * g + 1], cf[3 * g + 2]);
    return Cand{f2u(v) & 0x7fffffffu, g, v};
}
DWT_HD Cand better(const Cand &a, const Cand &b) { return (b.key > a.key || (b.key == a.key && b.g < a.g)) ? b : a; }

// the state of one slot (the DWT_SS_* words), held in registers between one load and one store
struct Slot {
    uint32_t cursor, held, n, seen, falls;
};
DWT_HD Slot load(const uint32_t *ss, int k, int s) {
    return Slot{ss[(size_t)DWT_SS_CURSOR * k + s], ss[(size_t)DWT_SS_HELD * k + s], ss[(size_t)DWT_SS_N * k + s], ss[(size_t)DWT_SS_SEEN * k + s],
                ss[(size_t)DWT_SS_FALLS * k + s]};
}
DWT_HD void store(uint32_t *ss, int k, int s, const Slot &t) {
    ss[(size_t)DWT_SS_CURSOR * k + s] = t.cursor; ss[(size_t)DWT_SS_HELD * k + s] = t.held; ss[(size_t)DWT_SS_N * k + s] = t.n;
    ss[(size_t)DWT_SS_SEEN * k + s] = t.seen; ss[(size_t)DWT_SS_FALLS * k + s] = t.falls;
}
DWT_HD void arm(Slot &t, int64_t progress) { t.cursor = t.held = t.seen = t.falls = 0u; t.n = (uint32_t)progress; }

// what one record decides for a slot that is not held
struct Step {
    uint32_t at;           // the ring row written
    uint32_t head[4];      // the row's integer words: DWT_CH_SEEN, DWT_CH_EPI_STEP, DWT_CH_FLAGS, DWT_CH_NAN_RESETS
};
static_assert(DWT_CH_SEEN == 0 && DWT_CH_EPI_STEP == 1 && DWT_CH_FLAGS == 2 && DWT_CH_NAN_RESETS == 3, "Step::head is row words 0..3");

// One record of a slot that is not held (t.seen already counts this call): the row's place and integer words, and the slot's next state.
// Terminal-row rule: after an in-step reset root_states, dof_state, target_vel and pert_on are the NEW episode's; contact_forces,
// action_torque and the rewards are the ended episode's; the row keeps them as the step left them.
DWT_HD Step advance(Slot &t, int depth, int hold_mode, bool reset, bool timeout, int pert_on, int pert_start, int nan_resets, float max_len) {
    Step o;
    const uint32_t n1 = t.n + 1u;
    const bool limit = (float)n1 >= max_len - 1.0f;
    o.at = t.cursor % (uint32_t)depth;
    o.head[DWT_CH_SEEN] = t.seen;
    o.head[DWT_CH_EPI_STEP] = n1;
    o.head[DWT_CH_FLAGS] = (reset ? DWT_FLAG_RESET : 0u) | (limit ? DWT_FLAG_TIME_LIMIT : 0u) | (pert_on ? DWT_FLAG_PERT_ON : 0u) |
                           (pert_start ? DWT_FLAG_PERT_START : 0u) | (timeout ? DWT_FLAG_TIMEOUT : 0u);
    o.head[DWT_CH_NAN_RESETS] = (uint32_t)nan_resets;
    t.cursor += 1u;
    if (t.cursor >= DWT_CURSOR_FOLD) t.cursor = (uint32_t)depth + t.cursor % (uint32_t)depth;          // (same row next, same full ring)
    if (reset) {
        if (!limit) t.falls += 1u;
        t.n = 0u;
        if (hold_mode == DWT_HOLD_RESET || (hold_mode == DWT_HOLD_FALL && !limit)) t.held = 1u;
    } else {
        t.n = n1;
    }
    return o;
}

// dwt_gather: row r (oldest first) of a slot with `cursor` rows written is ring row src_row(cursor, depth, r), for r < rows(cursor, depth)
DWT_HD uint32_t rows(uint32_t cursor, int depth) { return cursor < (uint32_t)depth ? cursor : (uint32_t)depth; }
DWT_HD uint32_t src_row(uint32_t cursor, int depth, uint32_t r) {
    return cursor <= (uint32_t)depth ? r : (cursor % (uint32_t)depth + r) % (uint32_t)depth;
}

}  // namespace dwt

#endif
