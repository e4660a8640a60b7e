// A g++ build of the forward dynamics' per-env arithmetic (isaacgymdyros_amd/csrc/dw_factor.h on top of dw_jacobian.h) with host pointers: the
// functions dw_forward_dynamics.hip runs, driven env by env in the kernel's order (every path of the tree, every record, every moving body,
// every pattern word of M, rows 38 down to 1 with every update of a row, the multipliers, every column).  tests/test_forward_dynamics.py
// compiles it and holds it against a float64 numpy restatement.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_factor.h"

extern "C" {

int dwlh_pack_table(const DwjModel *m, uint32_t *table, char *err, int errn) { return dwl::pack(m, table, err, (size_t)errn); }

// x [n][nrhs][39], factor, minv [n][39][39], each or NULL; rhs [n][nrhs][39], sub [n][39], mass_scale [n][38], dof_armature [n][33] or NULL.
// pattern_m [n][396] or NULL: the pattern words of M before the elimination (the tests hold them against the dense mass matrix)
int dwlh_solve(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale, const float *dof_armature,
               int vel_at_com, const float *rhs, int nrhs, const float *sub, float *x, float *factor, float *minv, float *pattern_m) {
    if (n < 1 || !table || !root_states || !dof_state || (rhs && !x) || (x && !rhs) || (sub && !rhs) || (rhs && (nrhs < 1 || nrhs > DWL_MAX_RHS)) ||
        (!x && !factor && !minv))
        return -1;
    const dwb::Tab T{table};
    for (int e = 0; e < n; ++e) {
        float E[dwl::ENV];
        memset(E, 0, sizeof(E));
        float *H = E + dwl::E_H;
        for (int l = 0; l < T.nleaf(); ++l) dwj::walk_path(T, l, root_states + (size_t)e * dwb::IN_ROOT, dof_state + (size_t)e * dwb::IN_DOF, vel_at_com, E);
        for (int k = 0; k < dwj::NI; ++k)
            dwj::record_inertia(T, E + dwj::E_KS, mass_scale ? mass_scale + (size_t)e * dwl::NB : nullptr, k, E + dwj::E_REC + k * dwj::RW);
        for (int i = 0; i < dwj::NM; ++i) dwj::body_sum(T, E, i);
        for (int p = 0; p < dwl::PAT; ++p) H[p] = dwl::form_word(T, E, dof_armature ? dof_armature + (size_t)e * DWL_NUM_DOF : nullptr, p);
        if (pattern_m) memcpy(pattern_m + (size_t)e * dwl::PAT, H, sizeof(float) * dwl::PAT);
        for (int k = dwl::NV - 1; k >= 1; --k)
            for (int s = 0; s < dwl::row_len(T, k) - 1; ++s)
                for (int t = 0; t <= s; ++t) {
                    int p;
                    const float v = dwl::eliminate_one(T, H, dwl::row_start(T, k), dwl::row_len(T, k), s, t, &p);
                    H[p] = v;
                }
        for (int p = 0; p < dwl::PAT; ++p) dwl::scale_word(T, H, p);
        if (factor)
            for (int i = 0; i < dwl::MMW; ++i) factor[(size_t)e * dwl::MMW + i] = dwl::factor_word(T, H, i / dwl::NV, i % dwl::NV);
        const int nid = minv ? dwl::NV : 0, ncol = nid + (x ? nrhs : 0);
        for (int c0 = 0; c0 < ncol; c0 += dwl::CAP) {
            const int nc = ncol - c0 < dwl::CAP ? ncol - c0 : dwl::CAP;
            for (int c = 0; c < nc; ++c)
                for (int k = 0; k < dwl::NV; ++k) {
                    const int col = c0 + c;
                    float v;
                    if (col < nid) {
                        v = k == col ? 1.0f : 0.0f;
                    } else {
                        v = rhs[((size_t)e * nrhs + (col - nid)) * dwl::NV + k];
                        v -= sub ? sub[(size_t)e * dwl::NV + k] : 0.0f;
                    }
                    E[c * dwl::NV + k] = v;
                }
            for (int c = 0; c < nc; ++c) dwl::solve_column(T, H, E + c * dwl::NV);
            for (int c = 0; c < nc; ++c) {
                const int col = c0 + c;
                if (col >= nid) memcpy(x + ((size_t)e * nrhs + (col - nid)) * dwl::NV, E + c * dwl::NV, sizeof(float) * dwl::NV);
            }
            if (c0 < nid)
                for (int i = 0; i < dwl::MMW; ++i) {
                    float v;
                    if (dwl::minv_word(E, c0, nid - c0 < nc ? nid - c0 : nc, i / dwl::NV, i % dwl::NV, &v)) minv[(size_t)e * dwl::MMW + i] = v;
                }
        }
    }
    return 0;
}

}  // extern "C"
