// A g++ build of the contact-consistent dynamics' per-env arithmetic (isaacgymdyros_amd/csrc/dw_contact.h on top of dw_factor.h, dw_dynamics.h
// and dw_jacobian.h) with host pointers: the functions dw_contact_dynamics.hip runs, driven env by env in the kernel's order (every path of the
// tree, every contact, every word of J_c, every record, every moving body, every pattern word of M, the elimination, the multipliers, the
// sweeps over the rows of J_c, A and its factor, x0, the small columns, the combination).  tests/test_contact_dynamics.py compiles it and holds
// it against a float64 numpy restatement.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_contact.h"

extern "C" {

int dwch_pack_table(const DwjModel *m, const DwcContacts *c, uint32_t *table, char *err, int errn) { return dwc::pack(m, c, table, err, (size_t)errn); }

// the outputs of dwc_solve, each or NULL; rhs [n][nrhs][39], sub [n][39], gamma [n][m], mass_scale [n][38], dof_armature [n][33] or NULL
int dwch_solve(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale, const float *dof_armature,
               int vel_at_com, const float *rhs, int nrhs, const float *sub, const float *gamma, float *jc, float *jdnu, float *minv_jt,
               float *lambda_inv, float *lambda, float *accel, float *force) {
    if (n < 1 || !table || !root_states || !dof_state || (rhs && !accel && !force) || ((accel || force) && !rhs) || (sub && !rhs) || (gamma && !rhs) ||
        (rhs && (nrhs < 1 || nrhs > DWC_MAX_RHS)) || (!jc && !jdnu && !minv_jt && !lambda_inv && !lambda && !accel && !force))
        return -1;
    const dwb::Tab T{table};
    const int K = dwc::count(T), m = 6 * K, NV = dwc::NV, AS = dwc::AS, R = rhs ? nrhs : 0;
    for (int e = 0; e < n; ++e) {
        float E[dwc::ENV];
        memset(E, 0, sizeof(E));
        float *H = E + dwl::E_H, *Y = E + dwc::E_Y, *A = E + dwc::E_A, *X0 = E + dwc::E_X0, *S = E + dwc::E_S;
        for (int l = 0; l < T.nleaf(); ++l)
            dwn::walk_path(T, l, root_states + (size_t)e * dwb::IN_ROOT, dof_state + (size_t)e * dwb::IN_DOF, nullptr, vel_at_com, E);
        for (int i = 0; i < K; ++i) dwc::contact_kin(T, E, i);
        for (int i = 0; i < m * NV; ++i) {
            const float v = dwc::jc_word(T, E, i / NV, i % NV);
            Y[i] = v;
            if (jc) jc[(size_t)e * m * NV + i] = v;
        }
        if (jdnu) memcpy(jdnu + (size_t)e * m, E + dwc::E_JD, sizeof(float) * m);
        if (!minv_jt && !lambda_inv && !lambda && !accel && !force) continue;
        for (int k = 0; k < dwj::NI; ++k)
            dwj::record_inertia(T, E + dwj::E_KS, mass_scale ? mass_scale + (size_t)e * dwc::NB : nullptr, k, E + dwj::E_REC + k * dwj::RW);
        for (int i = 0; i < dwj::NM; ++i) dwj::body_sum(T, E, i);
        for (int p = 0; p < dwl::PAT; ++p) H[p] = dwl::form_word(T, E, dof_armature ? dof_armature + (size_t)e * DWC_NUM_DOF : nullptr, p);
        for (int k = dwl::NV - 1; k >= 1; --k)
            for (int s = 0; s < dwl::row_len(T, k) - 1; ++s)
                for (int t = 0; t <= s; ++t) {
                    int p;
                    const float v = dwl::eliminate_one(T, H, dwl::row_start(T, k), dwl::row_len(T, k), s, t, &p);
                    H[p] = v;
                }
        for (int p = 0; p < dwl::PAT; ++p) dwl::scale_word(T, H, p);
        for (int r = 0; r < m; ++r) dwl::solve_column(T, H, Y + r * NV);
        for (int r = 0; r < m; ++r)
            for (int c = 0; c <= r; ++c) A[r * AS + c] = dwc::a_word(T, E, r, c);
        if (minv_jt) memcpy(minv_jt + (size_t)e * m * NV, Y, sizeof(float) * m * NV);
        if (lambda_inv)
            for (int i = 0; i < m * m; ++i) {
                const int r = i / m, c = i % m;
                lambda_inv[(size_t)e * m * m + i] = r >= c ? A[r * AS + c] : A[c * AS + r];
            }
        if (!lambda && !accel && !force) continue;
        for (int j = 0; j < m - 1; ++j)
            for (int i = j + 1; i < m; ++i)
                for (int k = j + 1; k <= i; ++k) dwc::ldl_one(A, j, i, k);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < i; ++j) dwc::ldl_scale(A, i, j);
        for (int c = 0; c < R; ++c) {
            for (int k = 0; k < NV; ++k) {
                float v = rhs[((size_t)e * R + c) * NV + k];
                v -= sub ? sub[(size_t)e * NV + k] : 0.0f;
                X0[c * NV + k] = v;
            }
            dwl::solve_column(T, H, X0 + c * NV);
        }
        const int nid = lambda ? m : 0, ncs = nid + R;
        for (int c = 0; c < ncs; ++c) {
            for (int i = 0; i < m; ++i)
                S[c * AS + i] = c < nid ? (i == c ? 1.0f : 0.0f) : dwc::g_word(T, E, gamma ? gamma + (size_t)e * m : nullptr, X0 + (c - nid) * NV, i);
        }
        for (int c = 0; c < ncs; ++c) dwc::small_solve(A, S + c * AS, m);
        if (lambda)
            for (int i = 0; i < m * m; ++i) lambda[(size_t)e * m * m + i] = dwc::mirror_word(S, i / m, i % m);
        for (int c = 0; c < R; ++c) {
            if (force) memcpy(force + ((size_t)e * R + c) * m, S + (nid + c) * AS, sizeof(float) * m);
            if (accel)
                for (int k = 0; k < NV; ++k) accel[((size_t)e * R + c) * NV + k] = dwc::accel_word(E, X0 + c * NV, S + (nid + c) * AS, m, k);
        }
    }
    return 0;
}

}  // extern "C"
