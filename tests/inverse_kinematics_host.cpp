// A g++ build of the inverse kinematics' per-env arithmetic (isaacgymdyros_amd/csrc/dw_inverse_kinematics.h on top of dw_jacobian.h and
// dw_contact.h) with host pointers: the functions dw_inverse_kinematics.hip runs, driven env by env in the kernel's order (dwq::solve_host:
// every path of the tree, every point, every error row, the status; J's words, A's folded triangle, the factor and the sweeps, dnu, the
// step limit, the update; one more walk at the end).  tests/test_inverse_kinematics.py compiles it and holds it against the float64 numpy
// reference of tests/inverse_kinematics_ref.py.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_inverse_kinematics.h"

extern "C" {

int dwqh_pack_table(const DwjModel *m, const DwcContacts *targets, const uint8_t *row_mask, const float *weights, const uint8_t *dof_mask,
                    const float *dof_lower, const float *dof_upper, const DwqParams *params, uint32_t *table, char *err, int errn) {
    return dwq::pack(m, targets, row_mask, weights, dof_mask, dof_lower, dof_upper, params, table, err, (size_t)errn);
}

// the outputs of dwq_solve, each or NULL; q0 [n][33] or NULL
int dwqh_solve(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *q0, const float *targets, float *q,
               float *root_out, float *residual, float *err, int32_t *iters, uint8_t *converged) {
    if (n < 1 || !table || !root_states || !dof_state || !targets) return -1;
    if (!q && !root_out && !residual && !err && !iters && !converged) return -1;
    const dwb::Tab T{table};
    const int K = dwq::count(T), m = 6 * K, ND = dwq::ND;
    for (int e = 0; e < n; ++e) {
        float E[dwq::ENV], root[dwb::IN_ROOT], dof[dwb::IN_DOF], tgt[dwq::MAXK * dwq::TW] = {0};
        memcpy(root, root_states + (size_t)e * dwb::IN_ROOT, sizeof(root));
        memcpy(dof, dof_state + (size_t)e * dwb::IN_DOF, sizeof(dof));
        memcpy(tgt, targets + (size_t)e * K * dwq::TW, sizeof(float) * K * dwq::TW);
        if (q0)
            for (int j = 0; j < ND; ++j) dof[2 * j] = q0[(size_t)e * ND + j];
        dwq::solve_host(T, E, root, dof, tgt);
        const bool dead = E[dwq::E_DEAD] != 0.0f;
        const float nan = NAN;
        if (q)
            for (int j = 0; j < ND; ++j) q[(size_t)e * ND + j] = dead ? nan : dof[2 * j];
        if (root_out)
            for (int c = 0; c < 7; ++c) root_out[(size_t)e * 7 + c] = dead ? nan : root[c];
        if (residual)
            for (int r = 0; r < m; ++r) residual[(size_t)e * m + r] = dead ? nan : E[dwq::E_ERR + r];
        if (err)
            for (int h = 0; h < 2; ++h) err[(size_t)e * 2 + h] = dead ? nan : dwq::err_max(T, E, K, h);
        if (iters) iters[e] = dead ? 0 : (int32_t)E[dwq::E_ITERS];
        if (converged) converged[e] = E[dwq::E_DONE] != 0.0f ? 1 : 0;
    }
    return 0;
}

}  // extern "C"
