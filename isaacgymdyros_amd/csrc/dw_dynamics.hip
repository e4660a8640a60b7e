// dw_dynamics.hip -- the kernel of the bias-force, gravity, inverse-dynamics and momentum tensors (include/dyros_dynamics.h; DESIGN.md
// section 24).  The per-env arithmetic is dw_dynamics.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both
// builds round alike.
// dwn_k_inverse_dynamics is shaped as dwj_k_mass_matrix is, with rows of 39 words where that one stores matrices: a workgroup of 256 lanes
// takes DWN_GROUP = 4 envs (an env's store is 7.7 KB of LDS: four of them, the table and the input rows are 38.5 KB, so four workgroups, 16
// waves, share a CU's 160 KB); the model table and the envs' input rows (contiguous blocks) come into LDS with consecutive lanes on consecutive
// words; a lane per (env, root-to-leaf path), packed into the first 32 lanes so that three of the four waves skip the phase, walks its path
// once and leaves, per moving body, pose, joint axis, velocities and the accelerations of nu_dot = 0 and of the caller's nu_dot; a lane per
// (env, record) leaves the record's COM offset, weight and (force, moment) pairs; a lane per (env, moving body) sums its subtree's pairs
// about its own origin through the subtree mask (no ordered upward pass) and leaves its word of every output row; last, the group's
// contiguous block of each output is written by consecutive lanes, 16 bytes per lane where the output is 16-byte aligned.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "dw_dynamics.h"
#include "dw_group.h"

namespace {

grp::Err s_err;

constexpr int G = DWN_GROUP, TPB = DWN_GROUP * DWN_LANES;
constexpr int IN_ROOT = dwb::IN_ROOT, IN_DOF = dwb::IN_DOF, NV = dwn::NV, NB = dwn::NB, ND = DWN_NUM_DOF;
static_assert(TPB % 64 == 0 && G * DWB_MAX_LEAVES <= 64, "whole waves, the paths of a group in one wave");
static_assert(G * dwn::NI <= TPB && G * dwn::NM <= TPB, "a lane per record, a lane per moving body");
static_assert((G * NV) % 4 == 0 && (G * DWN_MOM) % 4 == 0, "a group's blocks start on 16 bytes");
static_assert((DWN_TABLE_WORDS + G * (IN_ROOT + IN_DOF + NB + ND + NV + dwn::ENV)) * 4 <= 64 * 1024, "static LDS");

// the group's contiguous block of an output, rows of `row` words at word `at` of each env's OUT: 16 bytes per lane where dst is aligned
__device__ __forceinline__ void store_rows(float *__restrict__ dst, int e0, int ne, int row, int at, int t, const float *s_env) {
    grp::store_block<TPB>(dst + (size_t)e0 * row, ne * row, (reinterpret_cast<uintptr_t>(dst) & 15u) == 0u, t, [&](int idx) {
        const int e = idx / row;
        return s_env[e * dwn::ENV + dwn::E_OUT + at + (idx - row * e)];
    });
}

__global__ __launch_bounds__(TPB) void dwn_k_inverse_dynamics(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                              const float *__restrict__ dof_state, const float *__restrict__ mass_scale,
                                                              const float *__restrict__ dof_armature, float gx, float gy, float gz,
                                                              const float *__restrict__ accel, int vel_at_com, float *__restrict__ bias,
                                                              float *__restrict__ gravity, float *__restrict__ tau, float *__restrict__ momentum) {
    __shared__ uint4 s_tab4[DWN_TABLE_WORDS / 4];
    __shared__ float s_root[G * IN_ROOT];
    __shared__ float s_dof[G * IN_DOF];
    __shared__ float s_ms[G * NB];
    __shared__ float s_arm[G * ND];
    __shared__ float s_acc[G * NV];
    __shared__ float s_env[G * dwn::ENV];
    const int t = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = n - e0 < G ? n - e0 : G;          // envs of this workgroup (the last one may hold fewer)
    const int what = (bias != nullptr ? dwn::W_BIAS : 0) | (gravity != nullptr ? dwn::W_GRAV : 0) | (tau != nullptr && accel != nullptr ? dwn::W_TAU : 0) |
                     (momentum != nullptr ? dwn::W_MOM : 0);
    const bool has_acc = (what & dwn::W_TAU) != 0, has_ms = mass_scale != nullptr, has_arm = has_acc && dof_armature != nullptr;
    grp::load_table<TPB, DWN_TABLE_WORDS>(table, t, s_tab4);
    grp::load_rows<TPB>(root_states, e0, ne, IN_ROOT, t, s_root);
    grp::load_rows<TPB>(dof_state, e0, ne, IN_DOF, t, s_dof);
    if (has_ms) grp::load_rows<TPB>(mass_scale, e0, ne, NB, t, s_ms);
    if (has_arm) grp::load_rows<TPB>(dof_armature, e0, ne, ND, t, s_arm);
    if (has_acc) grp::load_rows<TPB>(accel, e0, ne, NV, t, s_acc);
    __syncthreads();
    const dwb::Tab T{reinterpret_cast<const uint32_t *>(s_tab4)};
    const float g[3] = {gx, gy, gz};
    const int nleaf = T.nleaf();
    if (nleaf > 0 && t < ne * nleaf) {
        const int ce = t / nleaf;
        dwn::walk_path(T, t - nleaf * ce, s_root + ce * IN_ROOT, s_dof + ce * IN_DOF, has_acc ? s_acc + ce * NV : nullptr, vel_at_com,
                       s_env + ce * dwn::ENV);
    }
    __syncthreads();
    if (t < ne * dwn::NI) {
        const int e = t / dwn::NI;
        dwn::record(T, s_env + e * dwn::ENV, has_ms ? s_ms + e * NB : nullptr, g, what, t - e * dwn::NI);
    }
    __syncthreads();
    // (body-major, leaves first: a wave's lanes hold bodies with subtrees of like size, and the wave that walked the chain starts on the leaves)
    if (t < ne * dwn::NM) {
        const int b = t / ne, e = t - b * ne;
        dwn::body_sum(T, s_env + e * dwn::ENV, has_arm ? s_arm + e * ND : nullptr, has_acc ? s_acc + e * NV : nullptr, g, what, dwn::NM - 1 - b);
    }
    __syncthreads();
    if (what & dwn::W_BIAS) store_rows(bias, e0, ne, NV, dwn::O_BIAS, t, s_env);
    if (what & dwn::W_GRAV) store_rows(gravity, e0, ne, NV, dwn::O_GRAV, t, s_env);
    if (what & dwn::W_TAU) store_rows(tau, e0, ne, NV, dwn::O_TAU, t, s_env);
    if (what & dwn::W_MOM) store_rows(momentum, e0, ne, DWN_MOM, dwn::O_MOM, t, s_env);
}

}  // namespace

extern "C" {

int dwn_abi_version(void) { return DWN_ABI_VERSION; }
const char *dwn_last_error(void) { return s_err.s; }

int dwn_pack_table(const DwjModel *m, uint32_t *table_host) { return dwj::pack(m, table_host, s_err.s, sizeof(s_err.s), "dwn_pack_table"); }

int dwn_inverse_dynamics(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
                         const float *dof_armature, float gx, float gy, float gz, const float *accel, int32_t vel_at_com, float *bias,
                         float *gravity, float *tau, float *momentum, void *stream) {
    if (num_envs < 1 || num_envs > 0x7fffffff / (IN_DOF + NV) - G) return s_err.fail("dwn_inverse_dynamics: num_envs must be in [1, 2^31 / 105 - 4)");
    if (!table || !root_states || !dof_state) return s_err.fail("dwn_inverse_dynamics: a buffer is missing");
    if ((reinterpret_cast<uintptr_t>(table) & 15u) != 0u) return s_err.fail("dwn_inverse_dynamics: the table must be 16-byte aligned");
    if (tau && !accel) return s_err.fail("dwn_inverse_dynamics: tau needs accel");
    if (!bias && !gravity && !tau && !momentum) return s_err.fail("dwn_inverse_dynamics: no output: nothing to compute");
    if (!isfinite(gx) || !isfinite(gy) || !isfinite(gz)) return s_err.fail("dwn_inverse_dynamics: the gravity vector is not finite");
    hipLaunchKernelGGL(dwn_k_inverse_dynamics, dim3(dwn::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs,
                       reinterpret_cast<const uint4 *>(table), root_states, dof_state, mass_scale, dof_armature, gx, gy, gz, accel,
                       (int)(vel_at_com != 0), bias, gravity, tau, momentum);
    return s_err.launched("dwn_inverse_dynamics");
}

}  // extern "C"
