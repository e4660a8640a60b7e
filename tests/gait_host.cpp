// A g++ build of the gait profile's per-env sample (isaacgymdyros_amd/csrc/dw_gait.h) with host pointers: the function dw_gait.hip runs,
// driven env by env into one [bins][DWG_W] table.  tests/test_gait_profile.py compiles it and holds it against a numpy restatement.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_gait.h"

namespace {
struct HostAdd {
    int64_t *table;
    void bin(int) const {}
    void add(int b, int w, int64_t v) const { table[b * dwg::W + w] += v; }
};
}  // namespace

extern "C" {

int dwgh_bins_ok(int bins) { return dwg::bins_ok(bins) ? 1 : 0; }
int dwgh_window_of(int idx) { return dwg::window_of(idx); }
int64_t dwgh_fx(double v) { return dwg::fx(v); }

// table [bins][DWG_W] and ct [DWG_CT_WORDS] are added to
int dwgh_record(int n, int bins, int min_episode_step, int skip_pushes, const float *root_states, const float *dof_state, const float *contact_forces,
                const float *env_state, const float *stacked_rewards, const int64_t *reset_buf, const int64_t *progress_buf, const float *total_mass,
                int64_t *table, int64_t *ct) {
    if (!dwg::bins_ok(bins) || n < 1 || min_episode_step < 0) return -1;
    const HostAdd a{table};
    for (int e = 0; e < n; ++e) {
        const float *es = env_state + (size_t)e * dwg::ESW;
        const float *cf = contact_forces + (size_t)e * DW_NUM_BODIES * 3;
        dwg::EnvIn in;
        in.fl = cf[3 * DWS_LFOOT + 2];
        in.fr = cf[3 * DWS_RFOOT + 2];
        in.total_mass = total_mass[e];
        in.tf0 = es[DW_ES_TARGET_FORCE];
        in.tf1 = es[DW_ES_TARGET_FORCE + 1];
        in.root_z = root_states[(size_t)e * 13 + 2];
        in.root_vx = root_states[(size_t)e * 13 + 7];
        in.tv0 = es[DW_ES_TARGET_VEL];
        in.paid = stacked_rewards[(size_t)e * DW_NUM_REW + DWG_PAID_COLUMN];
        in.dof_pos = dof_state + (size_t)e * 2 * DW_NUM_DOF;
        in.dof_stride = 2;
        in.tqpos = es + DW_ES_TARGET_QPOS;
        in.tq = es + DW_ES_ACTION_TORQUE;
        memcpy(&in.mocap_idx, es + DW_ES_MOCAP_IDX, 4);
        memcpy(&in.pert_on, es + DW_ES_PERT_ON, 4);
        in.reset = reset_buf[e] != 0;
        in.progress = progress_buf[e];
        ct[dwg::sample(in, bins, min_episode_step, skip_pushes != 0, a)] += 1;
    }
    return 0;
}

}  // extern "C"
