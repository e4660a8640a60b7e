// A g++ build of the foot force-torque sensors' per-env arithmetic (isaacgymdyros_amd/csrc/dw_sensors.h) with host pointers: the functions
// dw_sensors.hip runs, driven env by env in the kernel's order (both foot poses, then every output row).  tests/test_force_sensors.py
// compiles it and holds it against a float64 numpy restatement.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_sensors.h"

extern "C" {

int dwfh_pack_table(const DwbModel *m, uint32_t *table, char *err, int errn) { return dwb::pack(m, table, err, (size_t)errn); }

// sensors [n][ns][6], cop [n][2][4], zmp [n][4], corners [n][8][6]: each may be NULL; the refusals of dwf_refresh that need no device
int dwfh_refresh(int n, const uint32_t *table, const float *root_states, const float *dof_state, const float *env_state, const DwfModel *M,
                 const DwfSensor *S, int ns, float *sensors, float *cop, float *zmp, float *corners) {
    if (n < 1 || !table || !root_states || !dof_state || !env_state) return -1;
    if (dwf::refusal(M, S, ns) != nullptr) return -1;
    if ((ns > 0) != (sensors != nullptr) || (!sensors && !cop && !zmp && !corners)) return -1;
    const dwb::Tab T{table};
    for (int e = 0; e < n; ++e) {
        const float *root = root_states + (size_t)e * dwf::IN_ROOT, *dof = dof_state + (size_t)e * DWF_DOF_ROW;
        const float *warm = env_state + (size_t)e * DWF_ES_WORDS + DWF_ES_WARM;
        float fps[DWF_NUM_FEET * dwf::FP];
        for (int f = 0; f < DWF_NUM_FEET; ++f) dwf::foot_pose(T, M->foot_mv[f], root, dof, fps + f * dwf::FP);
        for (int s = 0; s < ns; ++s) dwf::sensor_row(*M, S[s], fps, warm, sensors + ((size_t)e * ns + s) * dwf::W_SEN);
        if (cop)
            for (int f = 0; f < DWF_NUM_FEET; ++f) dwf::cop_row(*M, f, warm, cop + (size_t)e * dwf::W_COP + f * DWF_COP_WORDS);
        if (zmp) dwf::zmp_row(*M, fps, warm, root, zmp + (size_t)e * dwf::W_ZMP);
        if (corners)
            for (int k = 0; k < dwf::NC; ++k) dwf::corner_row(*M, k, fps, warm, root, corners + (size_t)e * dwf::W_COR + k * DWF_CORNER_WORDS);
    }
    return 0;
}

}  // extern "C"
