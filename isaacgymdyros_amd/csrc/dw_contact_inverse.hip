// dw_contact_inverse.hip -- the kernel of the contact inverse dynamics (include/dyros_contact_inverse_dynamics.h).  The
// per-env arithmetic is dw_contact_inverse.h's on top of dw_dynamics.h and dw_jacobian.h, shared with a g++ build of the tests.  Built with
// -ffp-contract=off so that both builds round alike.
// dwi_k_solve is dwn_k_inverse_dynamics with a tail: a workgroup of 256 lanes takes DWI_GROUP = 4 envs; the table and the envs' input rows
// come into LDS; a lane per (env, path) walks the chain with the caller's nu_dot; a lane per (env, record) leaves the record's wrench while,
// in the last wave, a lane per (env, contact) forms the contact's point and J_c a + Jd_c nu; a lane per (env, moving body) sums its subtree
// to its word of r.  From there on a wave per env: G's 21 words and the six words of the right side with a lane each, the five columns of
// the factor and the two sweeps with a barrier between steps, f with a lane per row, tau_joint with a lane per joint.  The barriers are the
// workgroup's and stand outside divergent control flow: every loop bound comes from the table or is a constant, and `live` guards the work.
// An env's store is dw_dynamics.h's 7.7 KB and 108 words; a workgroup's LDS stays below a quarter of a CU's 160 KB, as dwn's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "dw_contact_inverse.h"
#include "dw_group.h"

namespace {

dwg::Err s_err;

constexpr int G = DWI_GROUP, L = DWI_LANES, TPB = DWI_GROUP * DWI_LANES;
constexpr int IN_ROOT = dwb::IN_ROOT, IN_DOF = dwb::IN_DOF, NV = dwi::NV, NB = dwi::NB, ND = dwi::ND, GN = dwi::GN, MAXM = dwi::MAXM;
static_assert(L == 64 && G * DWB_MAX_LEAVES <= 64, "a wave per env, the paths of a group in one wave");
static_assert(G * dwn::NI <= TPB - L && G * dwi::MAXK <= L && G * dwn::NM <= TPB, "the records leave the last wave to the contacts; a lane per moving body");
static_assert(dwi::GW + GN <= L && GN * GN <= L && MAXM <= L && NV <= L, "a lane per word of G and of its right side, per row, per joint");
static_assert((DWI_TABLE_WORDS + G * (IN_ROOT + IN_DOF + NB + ND + NV + dwi::ENV)) * 4 <= 160 * 1024 / 4, "four workgroups to a CU, as dwn");

__global__ __launch_bounds__(TPB) void dwi_k_solve(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                   const float *__restrict__ dof_state, const float *__restrict__ mass_scale,
                                                   const float *__restrict__ dof_armature, float gx, float gy, float gz,
                                                   const float *__restrict__ accel, const float *__restrict__ force_ref, int vel_at_com,
                                                   float *__restrict__ tau_joint, float *__restrict__ force, float *__restrict__ contact_accel,
                                                   float *__restrict__ tau_full) {
    __shared__ uint4 s_tab4[DWI_TABLE_WORDS / 4];
    __shared__ float s_root[G * IN_ROOT];
    __shared__ float s_dof[G * IN_DOF];
    __shared__ float s_ms[G * NB];
    __shared__ float s_arm[G * ND];
    __shared__ float s_acc[G * NV];
    __shared__ float s_env[G * dwi::ENV];
    const int t = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = n - e0 < G ? n - e0 : G;          // envs of this workgroup (the last one may hold fewer)
    const bool need_f = force != nullptr || tau_joint != nullptr, need_r = need_f || tau_full != nullptr;
    const int what = need_r ? dwn::W_TAU : 0;
    const bool has_acc = accel != nullptr, has_ms = mass_scale != nullptr, has_arm = has_acc && dof_armature != nullptr;
    dwg::load_table<TPB, DWI_TABLE_WORDS>(table, t, s_tab4);
    dwg::load_rows<TPB>(root_states, e0, ne, IN_ROOT, t, s_root);
    dwg::load_rows<TPB>(dof_state, e0, ne, IN_DOF, t, s_dof);
    if (has_ms && need_r) dwg::load_rows<TPB>(mass_scale, e0, ne, NB, t, s_ms);
    if (has_arm && need_r) dwg::load_rows<TPB>(dof_armature, e0, ne, ND, t, s_arm);
    if (has_acc) dwg::load_rows<TPB>(accel, e0, ne, NV, t, s_acc);
    __syncthreads();
    const dwb::Tab T{reinterpret_cast<const uint32_t *>(s_tab4)};
    const float g[3] = {gx, gy, gz};
    const int nleaf = T.nleaf(), K = dwi::count(T), m = 6 * K;
    // f_ref into the envs' stores (zeros when the caller has none: the same arithmetic, the same bits)
    if (need_f)
        for (int i = t; i < ne * m; i += TPB) {
            const int ce = i / m;
            s_env[ce * dwi::ENV + dwi::E_FR + (i - m * ce)] = force_ref != nullptr ? force_ref[(size_t)e0 * m + i] : 0.0f;
        }
    // a NULL nu_dot is zero: the walk then leaves the nu_dot = 0 words in the caller's slots as well
    if (nleaf > 0 && t < ne * nleaf) {
        const int ce = t / nleaf;
        dwn::walk_path(T, t - nleaf * ce, s_root + ce * IN_ROOT, s_dof + ce * IN_DOF, has_acc ? s_acc + ce * NV : nullptr, vel_at_com,
                       s_env + ce * dwi::ENV);
    }
    __syncthreads();
    if (need_r && t < ne * dwn::NI) {
        const int ce = t / dwn::NI;
        dwn::record(T, s_env + ce * dwi::ENV, has_ms ? s_ms + ce * NB : nullptr, g, what, t - ce * dwn::NI);
    }
    // (the last wave holds no record: its first lanes take the contacts)
    const int tc = t - (TPB - L);
    if (K > 0 && tc >= 0 && tc < ne * K) {
        const int ce = tc / K;
        dwi::contact_point(T, s_env + ce * dwi::ENV, tc - K * ce);
    }
    __syncthreads();
    if (need_r && t < ne * dwn::NM) {
        const int b = t / ne, ce = t - b * ne;
        dwn::body_sum(T, s_env + ce * dwi::ENV, has_arm ? s_arm + ce * ND : nullptr, has_acc ? s_acc + ce * NV : nullptr, g, what, dwn::NM - 1 - b);
    }
    __syncthreads();
    // from here on a wave per env
    const int e = t / L, lane = t - e * L;
    const bool live = e < ne;
    const size_t env = (size_t)(e0 + e);
    float *E = s_env + (live ? e : 0) * dwi::ENV, *Gm = E + dwi::E_G, *Y = E + dwi::E_Y;
    if (live) {
        if (contact_accel != nullptr && lane < m) contact_accel[env * m + lane] = E[dwi::E_CA + lane];
        if (tau_full != nullptr && lane < NV) tau_full[env * NV + lane] = E[dwi::E_TAU + lane];
    }
    if (!need_f) return;          // (every lane alike)
    if (live) {
        if (lane < dwi::GW) dwi::g_word(T, E, m, lane);
        else if (lane < dwi::GW + GN) dwi::y_word(T, E, m, lane - dwi::GW);
    }
    __syncthreads();
    // G = L D L': column j's updates read column j and write to its right
    for (int j = 0; j < GN - 1; ++j) {
        if (live && lane < GN * GN) {
            const int i = lane / GN, k = lane - GN * i;
            if (k > j && k <= i) dwi::ldl_one(Gm, j, i, k);
        }
        __syncthreads();
    }
    if (live && lane < GN * GN) {
        const int i = lane / GN, j = lane - GN * i;
        if (j < i) dwi::ldl_scale(Gm, i, j);
    }
    __syncthreads();
    for (int j = 0; j < GN - 1; ++j) {
        if (live && lane < GN && lane > j) dwi::sfwd_one(Gm, Y, j, lane);
        __syncthreads();
    }
    if (live && lane < GN) dwi::sscale_one(Gm, Y, lane);
    __syncthreads();
    for (int j = GN - 1; j >= 1; --j) {
        if (live && lane < j) dwi::sback_one(Gm, Y, j, lane);
        __syncthreads();
    }
    if (live && lane < m) {
        dwi::f_word(T, E, lane);
        if (force != nullptr) force[env * m + lane] = E[dwi::E_F + lane];
    }
    if (tau_joint == nullptr) return;
    __syncthreads();
    if (live && lane < ND) tau_joint[env * ND + lane] = dwi::tauj_word(T, E, K, lane);
}

}  // namespace

extern "C" {

int dwi_abi_version(void) { return DWI_ABI_VERSION; }
const char *dwi_last_error(void) { return s_err.s; }

int dwi_pack_table(const DwjModel *m, const DwcContacts *contacts, const float *weights, uint32_t *table_host) {
    return dwi::pack(m, contacts, weights, table_host, s_err.s, sizeof(s_err.s));
}

int dwi_solve(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
              const float *dof_armature, float gx, float gy, float gz, const float *accel, const float *force_ref, int32_t vel_at_com,
              float *tau_joint, float *force, float *contact_accel, float *tau_full, void *stream) {
    if (num_envs < 1 || num_envs > 0x7fffffff / (IN_DOF + NV) - G) return s_err.fail("dwi_solve: num_envs must be in [1, 2^31 / 105 - 4)");
    if (!table || !root_states || !dof_state) return s_err.fail("dwi_solve: a buffer is missing");
    if ((reinterpret_cast<uintptr_t>(table) & 15u) != 0u) return s_err.fail("dwi_solve: the table must be 16-byte aligned");
    if (!tau_joint && !force && !contact_accel && !tau_full) return s_err.fail("dwi_solve: no output: nothing to compute");
    if (!isfinite(gx) || !isfinite(gy) || !isfinite(gz)) return s_err.fail("dwi_solve: the gravity vector is not finite");
    hipLaunchKernelGGL(dwi_k_solve, dim3(dwn::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs,
                       reinterpret_cast<const uint4 *>(table), root_states, dof_state, mass_scale, dof_armature, gx, gy, gz, accel, force_ref,
                       (int)(vel_at_com != 0), tau_joint, force, contact_accel, tau_full);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : s_err.fail_hip("dwi_solve: launch", e);
}

}  // extern "C"
