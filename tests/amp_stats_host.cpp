// A g++ build of TocabiAMPLower's episode statistics' per-env update and reduction (isaacgymdyros_amd/csrc/dw_amp_stats.h) with host pointers:
// the same functions dw_amp_stats.hip runs, driven env by env.  tests/test_amp_episode_stats.py compiles it (with the host shims of tests/emul
// for the device-only headers it includes) and holds it against a numpy restatement.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_amp_stats.h"

namespace {
struct HostCount {
    uint64_t *w;
    void add(int k, uint32_t v) const { w[k] += v; }
    void max(int k, uint32_t v) const { if (v > w[k]) w[k] = v; }
};
}  // namespace

extern "C" {

int dweh_record(int n, const float *root_states, const float *contact_forces, const float *rigid_body_pos, const float *commands,
                const float *rew_buf, const float *reward_values, const int64_t *reset_buf, const int64_t *progress_buf, const float *total_mass,
                uint32_t *st, float *ac, uint64_t *ct, uint8_t *cause, float max_len, float term_h, int eet, float cmd_lo, float cmd_hi) {
    HostCount c{ct};
    dwe::Cfg C;
    C.max_len = max_len; C.term_h = term_h; C.cmd_lo = cmd_lo; C.cmd_hi = cmd_hi; C.eet = eet != 0;
    for (int e = 0; e < n; ++e) {
        const float *cf = contact_forces + (size_t)e * dwe::NB * 3, *bp = rigid_body_pos + (size_t)e * dwe::NB * 3;
        dwe::EnvIn in;
        in.root = root_states + (size_t)e * 13;
        in.rv = reward_values + (size_t)e * DWE_REW_TERMS;
        in.cmd = commands + (size_t)e * 3;
        in.fzl = cf[DWE_LFOOT * 3 + 2];
        in.fzr = cf[DWE_RFOOT * 3 + 2];
        in.zl = bp[DWE_LFOOT * 3 + 2];
        in.zr = bp[DWE_RFOOT * 3 + 2];
        in.rew = rew_buf[e];
        in.total_mass = total_mass[e];
        in.p = (int)progress_buf[e];
        in.reset = reset_buf[e] != 0;
        uint32_t lo, hi;
        dwe::contact_mask(cf, lo, hi);
        const dwe::Rows r{st, ac, n, e};
        dwe::St s = dwe::load(r);
        dwe::AcHot h = dwe::load_hot(r);
        int bin;
        cause[e] = (uint8_t)dwe::update(in, lo, hi, s, h, r, c, C, bin);
        dwe::store(r, s);
        dwe::store_hot(r, h, bin);
    }
    dwe::count_call(ct);
    return 0;
}

int dweh_summarize(int n, const float *ac, const uint64_t *ct, double *out) {
    for (int i = 0; i < DWE_CT_WORDS; ++i) out[i] = (double)ct[i];
    double red[dwe::RT];
    for (int k = 0; k < DWE_AC_WORDS; ++k) {
        for (int t = 0; t < dwe::RT; ++t) red[t] = dwe::partial(ac + (size_t)k * n, n, t);
        for (int s = dwe::RT / 2; s > 0; s >>= 1)
            for (int t = 0; t < s; ++t) red[t] += red[t + s];
        out[DWE_SUM_AC + k] = red[0];
    }
    return 0;
}

}  // extern "C"
