// A g++ build of the inverse dynamics' per-env arithmetic (isaacgymdyros_amd/csrc/dw_dynamics.h) with host pointers: the functions
// dw_dynamics.hip runs, driven env by env in the kernel's order (every path of the tree, every record, every moving body, every output
// row).  tests/test_dynamics.py compiles it and holds it against a float64 numpy restatement.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_dynamics.h"

extern "C" {

int dwnh_pack_table(const DwjModel *m, uint32_t *table, char *err, int errn) { return dwj::pack(m, table, err, (size_t)errn); }

// bias, gravity, tau [n][39], momentum [n][6], each or NULL; mass_scale [n][38], dof_armature [n][33], accel [n][39] or NULL
int dwnh_inverse_dynamics(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
                          const float *dof_armature, float gx, float gy, float gz, const float *accel, int vel_at_com, float *bias, float *gravity,
                          float *tau, float *momentum) {
    if (n < 1 || !table || !root_states || !dof_state || (tau && !accel) || (!bias && !gravity && !tau && !momentum)) return -1;
    const dwb::Tab T{table};
    const int what = (bias ? dwn::W_BIAS : 0) | (gravity ? dwn::W_GRAV : 0) | (tau ? dwn::W_TAU : 0) | (momentum ? dwn::W_MOM : 0);
    const float g[3] = {gx, gy, gz};
    for (int e = 0; e < n; ++e) {
        float E[dwn::ENV];
        memset(E, 0, sizeof(E));
        const float *acc = tau ? accel + (size_t)e * dwn::NV : nullptr;
        for (int l = 0; l < T.nleaf(); ++l)
            dwn::walk_path(T, l, root_states + (size_t)e * dwb::IN_ROOT, dof_state + (size_t)e * dwb::IN_DOF, acc, vel_at_com, E);
        for (int k = 0; k < dwn::NI; ++k) dwn::record(T, E, mass_scale ? mass_scale + (size_t)e * dwn::NB : nullptr, g, what, k);
        for (int i = 0; i < dwn::NM; ++i)
            dwn::body_sum(T, E, tau && dof_armature ? dof_armature + (size_t)e * DWN_NUM_DOF : nullptr, acc, g, what, i);
        const float *o = E + dwn::E_OUT;
        if (bias) memcpy(bias + (size_t)e * dwn::NV, o + dwn::O_BIAS, sizeof(float) * dwn::NV);
        if (gravity) memcpy(gravity + (size_t)e * dwn::NV, o + dwn::O_GRAV, sizeof(float) * dwn::NV);
        if (tau) memcpy(tau + (size_t)e * dwn::NV, o + dwn::O_TAU, sizeof(float) * dwn::NV);
        if (momentum) memcpy(momentum + (size_t)e * DWN_MOM, o + dwn::O_MOM, sizeof(float) * DWN_MOM);
    }
    return 0;
}

}  // extern "C"
