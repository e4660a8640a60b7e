// dw_jacobian.hip -- the kernels of the Jacobian and mass-matrix tensors (include/dyros_jacobians.h).  The per-env
// arithmetic is dw_jacobian.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
// Both kernels are store streams shaped as dwb_k_refresh is: a workgroup of 256 lanes takes DWJ_GROUP = 8 envs; the model table and the envs'
// input rows (contiguous blocks) come into LDS with consecutive lanes on consecutive words; a lane per (env, root-to-leaf path), packed into
// the first 40 lanes so that three of the four waves skip the phase, walks its path and leaves offset, quaternion and world joint axis of
// every moving body in LDS; last, the group's contiguous block of the output is written by consecutive lanes, 16 bytes per lane where the
// output is 16-byte aligned (a group's block then is too), every word formed from LDS on the way out.
//   dwj_k_jacobian     [ne * nb * 6 * 39] words.  With vel_at_com a lane per (env, inertial record) first leaves the record's COM offset.  A word is
//                      an ancestor-mask test, then +0.0, a stored axis component or one cross-product component.
//   dwj_k_mass_matrix  [ne * 39 * 39] words and optionally [ne * 3 * 39] of the COM Jacobian.  A lane per (env, record) leaves weight, COM and world
//                      rotational inertia; a lane per (env, moving body) sums the records of its subtree through the subtree mask (no ordered
//                      upward pass) and leaves, per row of M, that inertia applied to the row's unit motion; a word of the lower triangle is an
//                      ancestor-mask test and a six-term dot in one form for every block of M, mirrored above.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "dw_group.h"
#include "dw_jacobian.h"

namespace {

grp::Err s_err;

constexpr int G = DWJ_GROUP, TPB = DWJ_GROUP * DWJ_LANES;
constexpr int IN_ROOT = dwb::IN_ROOT, IN_DOF = dwb::IN_DOF;
static_assert(TPB % 64 == 0 && G * DWB_MAX_LEAVES <= 64, "whole waves, the paths of a group in one wave");
static_assert((G * IN_ROOT) % 4 == 0 && (G * dwj::JROW) % 4 == 0 && (G * dwj::MMW) % 4 == 0 && (G * dwj::CJW) % 4 == 0, "a group's blocks start on 16 bytes");
static_assert((DWJ_TABLE_WORDS + G * (IN_ROOT + IN_DOF + dwj::JAC_ENV + dwj::NB)) * 4 <= 64 * 1024, "static LDS, Jacobian");
static_assert((DWJ_TABLE_WORDS + G * (IN_ROOT + IN_DOF + dwj::NB + DWJ_NUM_DOF + dwj::MM_ENV)) * 4 <= 64 * 1024, "static LDS, mass matrix");

struct Ids {
    unsigned char b[40];
};

__global__ __launch_bounds__(TPB) void dwj_k_jacobian(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                      const float *__restrict__ dof_state, Ids ids, int nb, int vel_at_com, float *__restrict__ jac) {
    __shared__ uint4 s_tab4[DWJ_TABLE_WORDS / 4];
    __shared__ float s_root[G * IN_ROOT];
    __shared__ float s_dof[G * IN_DOF];
    __shared__ float s_env[G * dwj::JAC_ENV];
    __shared__ int s_rows[G * dwj::NB];          // the group's output rows resolved once: env << 25 | jac_row_of
    const int t = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = n - e0 < G ? n - e0 : G;          // envs of this workgroup (the last one may hold fewer)
    grp::load_table<TPB, DWJ_TABLE_WORDS>(table, t, s_tab4);
    grp::load_rows<TPB>(root_states, e0, ne, IN_ROOT, t, s_root);
    grp::load_rows<TPB>(dof_state, e0, ne, IN_DOF, t, s_dof);
    __syncthreads();
    const dwb::Tab T{reinterpret_cast<const uint32_t *>(s_tab4)};
    for (int i = t; i < ne * nb; i += TPB) {
        const int e = i / nb, g = ids.b[i - e * nb];
        s_rows[i] = dwj::jac_row_of(T, g < dwj::NB ? g : dwj::NB - 1, vel_at_com) | (e << 25);
    }
    const int nleaf = T.nleaf();
    if (nleaf > 0 && t < ne * nleaf) {
        const int ce = t / nleaf;
        dwj::walk_path(T, t - nleaf * ce, s_root + ce * IN_ROOT, s_dof + ce * IN_DOF, vel_at_com, s_env + ce * dwj::JAC_ENV);
    }
    __syncthreads();
    if (vel_at_com) {
        for (int i = t; i < ne * dwj::NI; i += TPB) {
            const int e = i / dwj::NI, k = i - e * dwj::NI;
            float R[9];
            float *E = s_env + e * dwj::JAC_ENV;
            dwj::record_com(T, E + dwj::E_KS, k, R, E + dwj::E_PC + 3 * k);
        }
        __syncthreads();
    }
    const int rw = nb * dwj::JROW;
    grp::store_block<TPB>(jac + (size_t)e0 * rw, ne * rw, (reinterpret_cast<uintptr_t>(jac) & 15u) == 0u, t, [&](int idx) {
        const int q = idx / dwj::NV, c = idx - dwj::NV * q, er = q / dwj::JR, i = q - dwj::JR * er;
        const int row = s_rows[er];
        return dwj::jac_word(T, s_env + (row >> 25) * dwj::JAC_ENV, row & 0x1ffffff, i, c);
    });
}

__global__ __launch_bounds__(TPB) void dwj_k_mass_matrix(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                         const float *__restrict__ dof_state, const float *__restrict__ mass_scale,
                                                         const float *__restrict__ dof_armature, int vel_at_com, float *__restrict__ mm,
                                                         float *__restrict__ com_jac) {
    __shared__ uint4 s_tab4[DWJ_TABLE_WORDS / 4];
    __shared__ float s_root[G * IN_ROOT];
    __shared__ float s_dof[G * IN_DOF];
    __shared__ float s_ms[G * dwj::NB];
    __shared__ float s_arm[G * DWJ_NUM_DOF];
    __shared__ float s_env[G * dwj::MM_ENV];
    const int t = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = n - e0 < G ? n - e0 : G;
    grp::load_table<TPB, DWJ_TABLE_WORDS>(table, t, s_tab4);
    grp::load_rows<TPB>(root_states, e0, ne, IN_ROOT, t, s_root);
    grp::load_rows<TPB>(dof_state, e0, ne, IN_DOF, t, s_dof);
    if (mass_scale != nullptr) grp::load_rows<TPB>(mass_scale, e0, ne, dwj::NB, t, s_ms);
    if (dof_armature != nullptr) grp::load_rows<TPB>(dof_armature, e0, ne, DWJ_NUM_DOF, t, s_arm);
    __syncthreads();
    const dwb::Tab T{reinterpret_cast<const uint32_t *>(s_tab4)};
    const int nleaf = T.nleaf();
    if (nleaf > 0 && t < ne * nleaf) {
        const int ce = t / nleaf;
        dwj::walk_path(T, t - nleaf * ce, s_root + ce * IN_ROOT, s_dof + ce * IN_DOF, vel_at_com, s_env + ce * dwj::MM_ENV);
    }
    __syncthreads();
    for (int i = t; i < ne * dwj::NI; i += TPB) {
        const int e = i / dwj::NI, k = i - e * dwj::NI;
        float *E = s_env + e * dwj::MM_ENV;
        dwj::record_inertia(T, E + dwj::E_KS, mass_scale != nullptr ? s_ms + e * dwj::NB : nullptr, k, E + dwj::E_REC + k * dwj::RW);
    }
    __syncthreads();
    // (body-major, leaves first: a wave's lanes hold bodies with subtrees of like size, and the wave that walked the chain starts on the leaves)
    for (int i = t; i < ne * dwj::NM; i += TPB) {
        const int b = i / ne;
        dwj::body_sum(T, s_env + (i - b * ne) * dwj::MM_ENV, dwj::NM - 1 - b);
    }
    __syncthreads();
    const bool arm = dof_armature != nullptr;
    grp::store_block<TPB>(mm + (size_t)e0 * dwj::MMW, ne * dwj::MMW, (reinterpret_cast<uintptr_t>(mm) & 15u) == 0u, t, [&](int idx) {
        const int e = idx / dwj::MMW, w = idx - dwj::MMW * e, r = w / dwj::NV;
        return dwj::mm_word(T, s_env + e * dwj::MM_ENV, arm ? s_arm + e * DWJ_NUM_DOF : nullptr, r, w - dwj::NV * r);
    });
    if (com_jac != nullptr)
        grp::store_block<TPB>(com_jac + (size_t)e0 * dwj::CJW, ne * dwj::CJW, (reinterpret_cast<uintptr_t>(com_jac) & 15u) == 0u, t, [&](int idx) {
            const int e = idx / dwj::CJW, w = idx - dwj::CJW * e, r = w / dwj::NV;
            return dwj::cj_word(T, s_env + e * dwj::MM_ENV, r, w - dwj::NV * r);
        });
}

int check_common(const char *who, int32_t num_envs, const void *table, const void *root_states, const void *dof_state, const void *out) {
    if (num_envs < 1 || num_envs > 0x7fffffff / (DWJ_NUM_BODIES * dwj::JROW) - G) return s_err.fail(who, "num_envs must be in [1, 2^31 / 8892 - 8)");
    if (!table || !root_states || !dof_state || !out) return s_err.fail(who, "a buffer is missing");
    if ((reinterpret_cast<uintptr_t>(table) & 15u) != 0u) return s_err.fail(who, "the table must be 16-byte aligned");
    return 0;
}

}  // namespace

extern "C" {

int dwj_abi_version(void) { return DWJ_ABI_VERSION; }
const char *dwj_last_error(void) { return s_err.s; }

int dwj_pack_table(const DwjModel *m, uint32_t *table_host) { return dwj::pack(m, table_host, s_err.s, sizeof(s_err.s)); }

int dwj_jacobian(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const int32_t *body_ids_host,
                 int32_t nb, int32_t vel_at_com, float *jac, void *stream) {
    if (check_common("dwj_jacobian", num_envs, table, root_states, dof_state, jac) != 0) return -1;
    Ids ids;
    if (body_ids_host == nullptr) {
        if (nb != 0 && nb != DWJ_NUM_BODIES) return s_err.fail("dwj_jacobian: without body ids nb must be 0 or 38");
        nb = DWJ_NUM_BODIES;
        for (int k = 0; k < 40; ++k) ids.b[k] = (unsigned char)(k < DWJ_NUM_BODIES ? k : 0);
    } else {
        if (nb < 1 || nb > DWJ_NUM_BODIES) return s_err.fail("dwj_jacobian: nb must be in 1..38");
        for (int k = 0; k < 40; ++k) ids.b[k] = 0;
        for (int k = 0; k < nb; ++k) {
            if (body_ids_host[k] < 0 || body_ids_host[k] >= DWJ_NUM_BODIES) return s_err.fail("dwj_jacobian: a body id is outside 0..37");
            ids.b[k] = (unsigned char)body_ids_host[k];
        }
    }
    hipLaunchKernelGGL(dwj_k_jacobian, dim3(dwj::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs,
                       reinterpret_cast<const uint4 *>(table), root_states, dof_state, ids, (int)nb, (int)(vel_at_com != 0), jac);
    return s_err.launched("dwj_jacobian");
}

int dwj_mass_matrix(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
                    const float *dof_armature, int32_t vel_at_com, float *mm, float *com_jac, void *stream) {
    if (check_common("dwj_mass_matrix", num_envs, table, root_states, dof_state, mm) != 0) return -1;
    hipLaunchKernelGGL(dwj_k_mass_matrix, dim3(dwj::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs,
                       reinterpret_cast<const uint4 *>(table), root_states, dof_state, mass_scale, dof_armature, (int)(vel_at_com != 0), mm, com_jac);
    return s_err.launched("dwj_mass_matrix");
}

}  // extern "C"
