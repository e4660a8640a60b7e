// A g++ build of the contact inverse dynamics' per-env arithmetic (isaacgymdyros_amd/csrc/dw_contact_inverse.h on top of dw_dynamics.h and
// dw_jacobian.h) with host pointers: the functions dw_contact_inverse.hip runs, driven env by env in the kernel's order (every path of the
// tree with nu_dot, every contact, every record, every moving body, G's words and the right side, the factor, the sweeps, f, tau_joint).
// tests/test_contact_inverse_dynamics.py compiles it and holds it against a float64 numpy restatement.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_contact_inverse.h"

extern "C" {

int dwih_pack_table(const DwjModel *m, const DwcContacts *c, const float *weights, uint32_t *table, char *err, int errn) {
    return dwi::pack(m, c, weights, table, err, (size_t)errn);
}

// the outputs of dwi_solve, each or NULL; accel [n][39], force_ref [n][m], mass_scale [n][38], dof_armature [n][33] or NULL
int dwih_solve(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale, const float *dof_armature,
               float gx, float gy, float gz, const float *accel, const float *force_ref, int vel_at_com, float *tau_joint, float *force,
               float *contact_accel, float *tau_full) {
    if (n < 1 || !table || !root_states || !dof_state || (!tau_joint && !force && !contact_accel && !tau_full)) return -1;
    if (!isfinite(gx) || !isfinite(gy) || !isfinite(gz)) return -1;
    const dwb::Tab T{table};
    const int K = dwi::count(T), m = 6 * K, NV = dwi::NV, ND = dwi::ND;
    const bool need_f = force || tau_joint, need_r = need_f || tau_full;
    const int what = need_r ? dwn::W_TAU : 0;
    const float g[3] = {gx, gy, gz};
    for (int e = 0; e < n; ++e) {
        float E[dwi::ENV];
        memset(E, 0, sizeof(E));
        const float *acc = accel ? accel + (size_t)e * NV : nullptr;
        for (int i = 0; i < m; ++i) E[dwi::E_FR + i] = force_ref ? force_ref[(size_t)e * m + i] : 0.0f;
        for (int l = 0; l < T.nleaf(); ++l)
            dwn::walk_path(T, l, root_states + (size_t)e * dwb::IN_ROOT, dof_state + (size_t)e * dwb::IN_DOF, acc, vel_at_com, E);
        if (need_r)
            for (int k = 0; k < dwn::NI; ++k) dwn::record(T, E, mass_scale ? mass_scale + (size_t)e * dwi::NB : nullptr, g, what, k);
        for (int i = 0; i < K; ++i) dwi::contact_point(T, E, i);
        if (need_r)
            for (int i = 0; i < dwn::NM; ++i) dwn::body_sum(T, E, acc && dof_armature ? dof_armature + (size_t)e * ND : nullptr, acc, g, what, i);
        if (contact_accel) memcpy(contact_accel + (size_t)e * m, E + dwi::E_CA, sizeof(float) * m);
        if (tau_full) memcpy(tau_full + (size_t)e * NV, E + dwi::E_TAU, sizeof(float) * NV);
        if (!need_f) continue;
        for (int u = 0; u < dwi::GW; ++u) dwi::g_word(T, E, m, u);
        for (int k = 0; k < dwi::GN; ++k) dwi::y_word(T, E, m, k);
        dwi::solve_host(T, E, m);
        if (force) memcpy(force + (size_t)e * m, E + dwi::E_F, sizeof(float) * m);
        if (tau_joint)
            for (int j = 0; j < ND; ++j) tau_joint[(size_t)e * ND + j] = dwi::tauj_word(T, E, K, j);
    }
    return 0;
}

}  // extern "C"
