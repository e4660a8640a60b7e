// A g++ build of the episode statistics' per-env update and reduction (isaacgymdyros_amd/csrc/dw_stats.h) with host pointers: the same
// functions dw_stats.hip runs, driven env by env.  tests/test_episode_stats.py compiles it and holds it against a numpy restatement.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_stats.h"

namespace {
struct HostCount {
    uint64_t *w;
    void add(int k, uint32_t v) const { w[k] += v; }
    void max(int k, uint32_t v) const { if (v > w[k]) w[k] = v; }
};
}  // namespace

extern "C" {

int dwsh_record(int n, const float *root_states, const float *contact_forces, const float *env_state, const int64_t *reset_buf,
                const float *total_mass, uint32_t *st, float *ac, uint64_t *ct, uint8_t *cause, float max_len, float dt_policy) {
    HostCount c{ct};
    for (int e = 0; e < n; ++e) {
        const float *es = env_state + (size_t)e * dws::ESW;
        int esi[DW_ES_WORDS];
        memcpy(esi, es, sizeof(esi));
        dws::EnvIn in;
        in.cf = contact_forces + (size_t)e * dws::NB * 3;
        in.root = root_states + (size_t)e * 13;
        in.tq = es + DW_ES_ACTION_TORQUE;
        in.tv0 = es[DW_ES_TARGET_VEL];
        in.tv1 = es[DW_ES_TARGET_VEL + 1];
        in.tf0 = es[DW_ES_TARGET_FORCE];
        in.tf1 = es[DW_ES_TARGET_FORCE + 1];
        in.last_return = es[DW_ES_LAST_RETURN];
        in.total_mass = total_mass[e];
        in.pert_on = esi[DW_ES_PERT_ON];
        in.nan_resets = esi[DW_ES_NAN_RESETS];
        in.reset = reset_buf[e] != 0;
        uint32_t lo, hi;
        dws::contact_mask(in.cf, lo, hi);
        const dws::Rows r{st, ac, n, e};
        dws::St s = dws::load(r);
        dws::AcHot h = dws::load_hot(r);
        cause[e] = (uint8_t)dws::update(in, lo, hi, s, h, r, c, max_len, dt_policy);
        dws::store(r, s);
        dws::store_hot(r, h);
    }
    int s0;
    memcpy(&s0, env_state + DW_ES_PERT_START, 4);
    dws::count_call(ct, s0);
    return 0;
}

int dwsh_restart(int n, const int32_t *ids, int num_ids, const float *root_states, const float *env_state, const int64_t *progress_buf, uint32_t *st) {
    const int m = ids ? num_ids : n;
    for (int i = 0; i < m; ++i) {
        const int e = ids ? ids[i] : i;
        if (e < 0 || e >= n) continue;
        const float *es = env_state + (size_t)e * dws::ESW;
        int po, nr;
        memcpy(&po, es + DW_ES_PERT_ON, 4);
        memcpy(&nr, es + DW_ES_NAN_RESETS, 4);
        dws::St s;
        dws::begin(s, (int)progress_buf[e], root_states + (size_t)e * 13, es[DW_ES_TARGET_VEL], po ? 1 : 0, nr);
        dws::store(dws::Rows{st, nullptr, n, e}, s);
    }
    return 0;
}

int dwsh_summarize(int n, const float *ac, const uint64_t *ct, double *out) {
    for (int i = 0; i < DWS_CT_WORDS; ++i) out[i] = (double)ct[i];
    double red[dws::RT];
    for (int k = 0; k < DWS_AC_WORDS; ++k) {
        for (int t = 0; t < dws::RT; ++t) red[t] = dws::partial(ac + (size_t)k * n, n, t);
        for (int s = dws::RT / 2; s > 0; s >>= 1)
            for (int t = 0; t < s; ++t) red[t] += red[t + s];
        out[DWS_SUM_AC + k] = red[0];
    }
    return 0;
}

}  // extern "C"
