// A g++ build of the Jacobians' and the mass matrix' per-env arithmetic (isaacgymdyros_amd/csrc/dw_jacobian.h) with host pointers: the
// functions dw_jacobian.hip runs, driven env by env in the kernels' order (every path of the tree, every record, every moving body, every
// output word).  tests/test_jacobians.py compiles it and holds it against a float64 numpy restatement.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_jacobian.h"

extern "C" {

int dwjh_pack_table(const DwjModel *m, uint32_t *table, char *err, int errn) { return dwj::pack(m, table, err, (size_t)errn); }

// jac [n][nb][6][39]; body_ids NULL: all 38 in order
int dwjh_jacobian(int n, const uint32_t *table, const float *root_states, const float *dof_state, const int32_t *body_ids, int nb, int vel_at_com,
                  float *jac) {
    if (n < 1 || !table || !root_states || !dof_state || !jac) return -1;
    if (!body_ids) nb = dwj::NB;
    if (nb < 1 || nb > dwj::NB) return -1;
    for (int k = 0; body_ids && k < nb; ++k)
        if (body_ids[k] < 0 || body_ids[k] >= dwj::NB) return -1;
    const dwb::Tab T{table};
    for (int e = 0; e < n; ++e) {
        float E[dwj::JAC_ENV];
        memset(E, 0, sizeof(E));
        for (int l = 0; l < T.nleaf(); ++l)
            dwj::walk_path(T, l, root_states + (size_t)e * dwb::IN_ROOT, dof_state + (size_t)e * dwb::IN_DOF, vel_at_com, E + dwj::E_KS);
        if (vel_at_com)
            for (int k = 0; k < dwj::NI; ++k) {
                float R[9];
                dwj::record_com(T, E + dwj::E_KS, k, R, E + dwj::E_PC + 3 * k);
            }
        for (int r = 0; r < nb; ++r) {
            const int row = dwj::jac_row_of(T, body_ids ? body_ids[r] : r, vel_at_com);
            for (int i = 0; i < dwj::JR; ++i)
                for (int c = 0; c < dwj::NV; ++c) jac[(((size_t)e * nb + r) * dwj::JR + i) * dwj::NV + c] = dwj::jac_word(T, E, row, i, c);
        }
    }
    return 0;
}

// mm [n][39][39], com_jac [n][3][39] or NULL; mass_scale [n][38] and dof_armature [n][33] or NULL
int dwjh_mass_matrix(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
                     const float *dof_armature, int vel_at_com, float *mm, float *com_jac) {
    if (n < 1 || !table || !root_states || !dof_state || !mm) return -1;
    const dwb::Tab T{table};
    for (int e = 0; e < n; ++e) {
        float E[dwj::MM_ENV];
        memset(E, 0, sizeof(E));
        for (int l = 0; l < T.nleaf(); ++l)
            dwj::walk_path(T, l, root_states + (size_t)e * dwb::IN_ROOT, dof_state + (size_t)e * dwb::IN_DOF, vel_at_com, E + dwj::E_KS);
        for (int k = 0; k < dwj::NI; ++k)
            dwj::record_inertia(T, E + dwj::E_KS, mass_scale ? mass_scale + (size_t)e * dwj::NB : nullptr, k, E + dwj::E_REC + k * dwj::RW);
        for (int i = 0; i < dwj::NM; ++i) dwj::body_sum(T, E, i);
        const float *arm = dof_armature ? dof_armature + (size_t)e * DWJ_NUM_DOF : nullptr;
        for (int r = 0; r < dwj::NV; ++r)
            for (int c = 0; c < dwj::NV; ++c) mm[((size_t)e * dwj::NV + r) * dwj::NV + c] = dwj::mm_word(T, E, arm, r, c);
        if (com_jac)
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < dwj::NV; ++c) com_jac[((size_t)e * 3 + r) * dwj::NV + c] = dwj::cj_word(T, E, r, c);
    }
    return 0;
}

}  // extern "C"
