// A g++ build of the contact and the stance inverse dynamics' per-env arithmetic (isaacgymdyros_amd/csrc/dw_contact_inverse.h and
// dw_stance_inverse.h on top of dw_dynamics.h and dw_jacobian.h) with host pointers: the functions dw_contact_inverse.hip runs, driven env by
// env in the kernel's order (every path of the tree with nu_dot, every contact, every record, every moving body, the mask, G's words and the
// right side, the factor and the sweeps where the stance is not empty, f, tau_joint, base_residual, margins, feasible).
// tests/test_contact_inverse_dynamics.py and tests/test_stance_inverse_dynamics.py compile it and hold it against float64 numpy restatements.
// dwkh_solve and dwih_solve_product (every contact on) run the product's sums, contact by contact over a mask; dwih_solve runs section 27's
// plain statement of the same sums, row-ascending and without a mask, which stands in this file only (namespace plain): the tests hold the
// one against the other bit for bit.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_stance_inverse.h"

namespace plain {

using namespace dwi;

// word u = 0 .. 20 of G's lower triangle, (i, j) with i >= j, row after row: the rows of J_b ascending
void g_word(const Tab &T, float *E, int m, int u) {
    const int i = u < 1 ? 0 : (u < 3 ? 1 : (u < 6 ? 2 : (u < 10 ? 3 : (u < 15 ? 4 : 5)))), j = u - i * (i + 1) / 2;
    float v = 0.0f;
    for (int r = 0; r < m; ++r) v += (jc_word(T, E, r, i) / weight(T, r)) * jc_word(T, E, r, j);
    E[E_G + i * GS + j] = v;
    E[E_G + j * GS + i] = v;
}

// word k of the right side of G y = r[0:6] - J_b' f_ref, in that order
void y_word(const Tab &T, float *E, int m, int k) {
    float s = 0.0f;
    for (int r = 0; r < m; ++r) s += jc_word(T, E, r, k) * E[E_FR + r];
    E[E_Y + k] = E[E_TAU + k] - s;
}

// word r of f = f_ref + W^-1 J_b y
void f_word(const Tab &T, float *E, int r) {
    float s = 0.0f;
    for (int k = 0; k < GN; ++k) s += jc_word(T, E, r, k) * E[E_Y + k];
    E[E_F + r] = E[E_FR + r] + s / weight(T, r);
}

// tau_joint[j] = r[6 + j] - J_j' f: the contacts that have joint j on their path, ascending
float tauj_word(const Tab &T, const float *E, int K, int j) {
    float s = 0.0f;
    for (int i = 0; i < K; ++i) {
        const int b = body(T, i);
        if (!dwj::bit(T, DWJ_T_ANC, b, j + 1)) continue;
        for (int w = 0; w < 6; ++w) s += dwj::jac_word(T, E, b | ((E_PT + 3 * i) << 8), w, 6 + j) * E[E_F + 6 * i + w];
    }
    return E[E_TAU + 6 + j] - s;
}

}  // namespace plain

namespace {

// every env in turn.  PLAIN: section 27's row-ordered sums, no stance; otherwise the product's, over each env's mask (stance NULL: every contact)
template <bool PLAIN>
int solve(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale, const float *dof_armature, float gx,
          float gy, float gz, const float *accel, const float *force_ref, const uint8_t *stance, int vel_at_com, float *tau_joint, float *force,
          float *contact_accel, float *tau_full, float *base_residual, float *margins, uint8_t *feasible) {
    if (n < 1 || !table || !root_states || !dof_state) return -1;
    if (!tau_joint && !force && !contact_accel && !tau_full && !base_residual && !margins && !feasible) return -1;
    if (!isfinite(gx) || !isfinite(gy) || !isfinite(gz)) return -1;
    const dwb::Tab T{table};
    const int K = dwi::count(T), m = 6 * K, NV = dwi::NV, ND = dwi::ND;
    const bool need_f = force || tau_joint || base_residual || margins || feasible, need_r = need_f || tau_full;
    const int what = need_r ? dwn::W_TAU : 0;
    const float g[3] = {gx, gy, gz};
    for (int e = 0; e < n; ++e) {
        float E[dwi::ENV];
        memset(E, 0, sizeof(E));
        const float *acc = accel ? accel + (size_t)e * NV : nullptr;
        const uint32_t mask = dwk::mask_of(stance ? stance + (size_t)e * K : nullptr, K);
        for (int i = 0; i < m; ++i) E[dwi::E_FR + i] = force_ref && dwk::on(mask, i / 6) ? force_ref[(size_t)e * m + i] : 0.0f;
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
        if (PLAIN) {
            for (int u = 0; u < dwi::GW; ++u) plain::g_word(T, E, m, u);
            for (int k = 0; k < dwi::GN; ++k) plain::y_word(T, E, m, k);
            dwi::factor_host(E);
            for (int r = 0; r < m; ++r) plain::f_word(T, E, r);
        } else {
            if (mask != 0u) {
                for (int u = 0; u < dwi::GW; ++u) dwi::g_word(T, E, K, mask, u);
                for (int k = 0; k < dwi::GN; ++k) dwi::y_word(T, E, K, mask, k);
            }
            dwi::solve_host(T, E, K, mask);
        }
        if (force) memcpy(force + (size_t)e * m, E + dwi::E_F, sizeof(float) * m);
        if (tau_joint)
            for (int j = 0; j < ND; ++j) tau_joint[(size_t)e * ND + j] = PLAIN ? plain::tauj_word(T, E, K, j) : dwi::tauj_word(T, E, K, mask, j);
        if (base_residual)
            for (int k = 0; k < dwi::GN; ++k) base_residual[(size_t)e * dwi::GN + k] = dwk::base_word(T, E, K, mask, k);
        if (margins)
            for (int i = 0; i < K; ++i) dwk::margins4(T, E, mask, i, margins + ((size_t)e * K + i) * dwk::MW);
        if (feasible) feasible[e] = dwk::feasible_of(T, E, K, mask);
    }
    return 0;
}

}  // namespace

extern "C" {

int dwih_pack_table(const DwjModel *m, const DwcContacts *c, const float *weights, uint32_t *table, char *err, int errn) {
    return dwi::pack(m, c, weights, table, err, (size_t)errn);
}

int dwkh_pack_table(const DwjModel *m, const DwcContacts *c, const float *weights, const float *soles, float mu, uint32_t *table, char *err, int errn) {
    return dwk::pack(m, c, weights, soles, mu, table, err, (size_t)errn);
}

// the outputs of dwi_solve, each or NULL; accel [n][39], force_ref [n][m], mass_scale [n][38], dof_armature [n][33] or NULL: the plain sums
int dwih_solve(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale, const float *dof_armature,
               float gx, float gy, float gz, const float *accel, const float *force_ref, int vel_at_com, float *tau_joint, float *force,
               float *contact_accel, float *tau_full) {
    return solve<true>(n, table, root_states, dof_state, mass_scale, dof_armature, gx, gy, gz, accel, force_ref, nullptr, vel_at_com, tau_joint, force,
                       contact_accel, tau_full, nullptr, nullptr, nullptr);
}

// the same by the product's sums with every contact on: what dwi_solve runs
int dwih_solve_product(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale, const float *dof_armature,
                       float gx, float gy, float gz, const float *accel, const float *force_ref, int vel_at_com, float *tau_joint, float *force,
                       float *contact_accel, float *tau_full) {
    return solve<false>(n, table, root_states, dof_state, mass_scale, dof_armature, gx, gy, gz, accel, force_ref, nullptr, vel_at_com, tau_joint, force,
                        contact_accel, tau_full, nullptr, nullptr, nullptr);
}

// the outputs of dwk_solve, each or NULL; stance [n][K] or NULL (every contact)
int dwkh_solve(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale, const float *dof_armature,
               float gx, float gy, float gz, const float *accel, const float *force_ref, const uint8_t *stance, int vel_at_com, float *tau_joint,
               float *force, float *contact_accel, float *tau_full, float *base_residual, float *margins, uint8_t *feasible) {
    return solve<false>(n, table, root_states, dof_state, mass_scale, dof_armature, gx, gy, gz, accel, force_ref, stance, vel_at_com, tau_joint, force,
                        contact_accel, tau_full, base_residual, margins, feasible);
}

}  // extern "C"
