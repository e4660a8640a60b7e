// A g++ build of the run trace's row assembly and slot state (isaacgymdyros_amd/csrc/dw_trace.h) with host pointers: the same functions
// dw_trace.hip runs, driven slot by slot.  tests/test_run_trace.py compiles it and holds it against a numpy restatement.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_trace.h"

extern "C" {

int dwth_record(int n, int k, int depth, int hold_mode, const int32_t *slot_env, const float *root_states, const float *dof_state,
                const float *contact_forces, const float *env_state, const float *rew_buf, const float *stacked_rewards,
                const int64_t *reset_buf, const int64_t *timeout_buf, float max_len, uint32_t *ss, uint32_t *ring) {
    for (int s = 0; s < k; ++s) {
        const int e = slot_env[s];
        if (e < 0 || e >= n) continue;
        dwt::Slot t = dwt::load(ss, k, s);
        t.seen += 1u;
        if (t.held != 0u) {
            ss[(size_t)DWT_SS_SEEN * k + s] = t.seen;
            continue;
        }
        const dwt::Src src = dwt::rows_of(e, root_states, dof_state, env_state, rew_buf, stacked_rewards);
        float row[DWT_ROW_WORDS];
        for (int q = 0; q < dwt::NSPAN; ++q) {
            const dwt::Span sp = dwt::span(q);
            for (int i = 0; i < sp.len; ++i) row[dwt::dst_of(sp, i)] = src.p[sp.buf][sp.src + i];
        }
        const float *cf = contact_forces + (size_t)e * dwt::CFW;
        int esi[DW_ES_WORDS];
        memcpy(esi, src.p[dwt::B_ES], sizeof(esi));
        const dwt::Step o = dwt::advance(t, depth, hold_mode, reset_buf[e] != 0, timeout_buf[e] != 0, esi[DW_ES_PERT_ON], esi[DW_ES_PERT_START],
                                         esi[DW_ES_NAN_RESETS], max_len);
        for (int i = 0; i < 4; ++i) row[i] = dwt::u2f(o.head[i]);
        for (int i = 0; i < DWT_LEN_PAD; ++i) row[DWT_CH_PAD + i] = 0.0f;
        dwt::Cand c = dwt::no_cand();
        for (int g = dwt::NB - 1; g >= 0; --g) c = dwt::better(c, dwt::cand_of(cf, g));          // (any order: the candidates are totally ordered)
        for (int i = 0; i < 3; ++i) {
            row[DWT_CH_FOOT_FORCE + i] = cf[3 * DWS_LFOOT + i];
            row[DWT_CH_FOOT_FORCE + 3 + i] = cf[3 * DWS_RFOOT + i];
        }
        row[DWT_CH_NF_MAX] = c.v;
        row[DWT_CH_NF_BODY] = (float)c.g;
        memcpy(ring + ((size_t)s * depth + o.at) * DWT_ROW_WORDS, row, sizeof(row));
        dwt::store(ss, k, s, t);
    }
    return 0;
}

int dwth_arm(int n, int k, const int32_t *ids, int num_ids, const int64_t *progress_buf, const int32_t *env_slot, uint32_t *ss) {
    const int m = ids ? num_ids : n;
    for (int i = 0; i < m; ++i) {
        const int e = ids ? ids[i] : i;
        if (e < 0 || e >= n) continue;
        const int s = env_slot[e];
        if (s < 0 || s >= k) continue;
        dwt::Slot t;
        dwt::arm(t, progress_buf[e]);
        dwt::store(ss, k, s, t);
    }
    return 0;
}

int dwth_gather(int k, int depth, const int32_t *slot_ids, int num_ids, const uint32_t *ss, const uint32_t *ring, uint32_t *out, int32_t *out_rows) {
    for (int i = 0; i < num_ids; ++i) {
        const int s = slot_ids ? slot_ids[i] : i;
        const bool ok = s >= 0 && s < k;
        const uint32_t cursor = ok ? ss[(size_t)DWT_SS_CURSOR * k + s] : 0u, nr = dwt::rows(cursor, depth);
        out_rows[i] = (int32_t)nr;
        for (uint32_t r = 0; r < (uint32_t)depth; ++r) {
            uint32_t *dst = out + ((size_t)i * depth + r) * DWT_ROW_WORDS;
            if (r < nr) memcpy(dst, ring + ((size_t)s * depth + dwt::src_row(cursor, depth, r)) * DWT_ROW_WORDS, 4 * DWT_ROW_WORDS);
            else memset(dst, 0, 4 * DWT_ROW_WORDS);
        }
    }
    return 0;
}

}  // extern "C"
