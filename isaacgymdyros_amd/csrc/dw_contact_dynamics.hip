// dw_contact_dynamics.hip -- the kernel of the contact-consistent dynamics (include/dyros_contact_dynamics.h).  The
// per-env arithmetic is dw_contact.h's on top of dw_factor.h, dw_dynamics.h and dw_jacobian.h, shared with a g++ build of the tests.  Built
// with -ffp-contract=off so that both builds round alike.
// dwc_k_solve's front end is dwl_k_solve's with dw_dynamics.h's chain walk: a workgroup of 192 lanes takes DWC_GROUP = 3 envs, a wave each; the
// table and the envs' input rows come into LDS; a lane per (env, path) walks the chain, which leaves every body's velocity and acceleration at
// nu_dot = 0 where the mass matrix's records go later, so a lane per (env, contact) forms the contact's point and Jd_c nu first, and the env's
// wave writes J_c into Y, a store of its own where dwl's sweeps solve its rows in place (J_c itself is not kept: dw_contact.h forms its words
// again from the chain's words, which stay to the end).  Then dwl_k_solve's records, subtree sums, pattern words, elimination and multipliers
// (dw_factor_wave.h's stages, one definition for both kernels);
// the sweeps over Y; A = J_c Y (rows >= columns) and its dense L D L', a column's updates spread over the wave with a barrier between columns;
// x0 behind the chain's words; the small columns (the identity's for A^-1, the right sides of A f = g) swept side by side; nu_dot = x0 + Y f.
// An env's store is 12.1 KB, a workgroup's LDS 46 KB: three workgroups, nine envs, share a CU's 160 KB.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "dw_contact.h"
#include "dw_factor_wave.h"
#include "dw_group.h"

namespace {

grp::Err s_err;

constexpr int G = DWC_GROUP, L = DWC_LANES, TPB = DWC_GROUP * DWC_LANES;
constexpr int IN_ROOT = dwb::IN_ROOT, IN_DOF = dwb::IN_DOF, NV = dwc::NV, NB = dwc::NB, ND = DWC_NUM_DOF, AS = dwc::AS, MAXM = dwc::MAXM;
static_assert(L == dwl::L && G * DWB_MAX_LEAVES <= 64, "a wave per env, the paths of a group in one wave");
static_assert(G * dwj::NI <= TPB && G * dwj::NM <= TPB && G * dwc::MAXK <= TPB, "a lane per record, per moving body, per contact");
static_assert((DWC_TABLE_WORDS + G * (IN_ROOT + IN_DOF + NB + ND + dwc::ENV)) * 4 <= 64 * 1024, "static LDS");

__global__ __launch_bounds__(TPB) void dwc_k_solve(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                   const float *__restrict__ dof_state, const float *__restrict__ mass_scale,
                                                   const float *__restrict__ dof_armature, int vel_at_com, const float *__restrict__ rhs, int nrhs,
                                                   const float *__restrict__ sub, const float *__restrict__ gamma, float *__restrict__ jc,
                                                   float *__restrict__ jdnu, float *__restrict__ minv_jt, float *__restrict__ lambda_inv,
                                                   float *__restrict__ lambda, float *__restrict__ accel, float *__restrict__ force) {
    __shared__ uint4 s_tab4[DWC_TABLE_WORDS / 4];
    __shared__ float s_root[G * IN_ROOT];
    __shared__ float s_dof[G * IN_DOF];
    __shared__ float s_ms[G * NB];
    __shared__ float s_arm[G * ND];
    __shared__ float s_env[G * dwc::ENV];
    const int t = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = n - e0 < G ? n - e0 : G;          // envs of this workgroup (the last one may hold fewer)
    const bool has_ms = mass_scale != nullptr, has_arm = dof_armature != nullptr;
    grp::load_table<TPB, DWC_TABLE_WORDS>(table, t, s_tab4);
    grp::load_rows<TPB>(root_states, e0, ne, IN_ROOT, t, s_root);
    grp::load_rows<TPB>(dof_state, e0, ne, IN_DOF, t, s_dof);
    if (has_ms) grp::load_rows<TPB>(mass_scale, e0, ne, NB, t, s_ms);
    if (has_arm) grp::load_rows<TPB>(dof_armature, e0, ne, ND, t, s_arm);
    __syncthreads();
    const dwb::Tab T{reinterpret_cast<const uint32_t *>(s_tab4)};
    const int nleaf = T.nleaf(), K = dwc::count(T), m = 6 * K;
    if (nleaf > 0 && t < ne * nleaf) {
        const int ce = t / nleaf;
        dwn::walk_path(T, t - nleaf * ce, s_root + ce * IN_ROOT, s_dof + ce * IN_DOF, nullptr, vel_at_com, s_env + ce * dwc::ENV);
    }
    __syncthreads();
    if (K > 0 && t < ne * K) {
        const int ce = t / K;
        dwc::contact_kin(T, s_env + ce * dwc::ENV, t - K * ce);
    }
    __syncthreads();
    // from here on a wave per env; the barriers are the workgroup's, every loop bound is the same for every env
    const int e = t / L, lane = t - e * L;
    const bool live = e < ne;
    const size_t env = (size_t)(e0 + e);
    float *E = s_env + (live ? e : 0) * dwc::ENV, *H = E + dwl::E_H, *Y = E + dwc::E_Y, *A = E + dwc::E_A;
    if (live) {
        for (int i = lane; i < m * NV; i += L) {
            const int r = i / NV;
            const float v = dwc::jc_word(T, E, r, i - NV * r);
            Y[i] = v;
            if (jc != nullptr) jc[env * m * NV + i] = v;
        }
        if (jdnu != nullptr)
            for (int i = lane; i < m; i += L) jdnu[env * m + i] = E[dwc::E_JD + i];
    }
    if (minv_jt == nullptr && lambda_inv == nullptr && lambda == nullptr && accel == nullptr && force == nullptr) return;          // (every lane alike)
    __syncthreads();
    dwl::inertia<dwc::ENV>(T, s_env, has_ms, s_ms, ne, t);
    dwl::form(T, E, H, has_arm ? s_arm + e * ND : nullptr, lane, live);
    dwl::eliminate(T, H, lane, live);
    // Y = M^-1 J_c', the rows in place
    dwl::sweeps(T, H, Y, m, lane, live);
    if (live) {
        for (int i = lane; i < m * m; i += L) {
            const int r = i / m, c = i - m * r;
            if (c <= r) A[r * AS + c] = dwc::a_word(T, E, r, c);
        }
        if (minv_jt != nullptr)
            for (int i = lane; i < m * NV; i += L) minv_jt[env * m * NV + i] = Y[i];
    }
    __syncthreads();
    if (live && lambda_inv != nullptr)
        for (int i = lane; i < m * m; i += L) {
            const int r = i / m, c = i - m * r;
            lambda_inv[env * m * m + i] = r >= c ? A[r * AS + c] : A[c * AS + r];
        }
    if (lambda == nullptr && accel == nullptr && force == nullptr) return;
    __syncthreads();
    // A = L D L': column j's updates read column j and write to its right
    for (int j = 0; j < m - 1; ++j) {
        if (live)
            for (int u = lane; u < m * m; u += L) {
                const int i = u / m, k = u - m * i;
                if (k > j && k <= i) dwc::ldl_one(A, j, i, k);
            }
        __syncthreads();
    }
    if (live)
        for (int u = lane; u < m * m; u += L) {
            const int i = u / m, j = u - m * i;
            if (j < i) dwc::ldl_scale(A, i, j);
        }
    __syncthreads();
    // x0 = M^-1 (rhs - sub) in the front end's store
    const int R = rhs != nullptr ? nrhs : 0;
    float *X0 = E + dwc::E_X0, *S = E + dwc::E_S;
    if (R > 0) {
        if (live)
            for (int i = lane; i < R * NV; i += L) {
                const int c = i / NV, k = i - NV * c;
                float v = rhs[(env * R + c) * NV + k];
                v -= sub != nullptr ? sub[env * NV + k] : 0.0f;
                X0[i] = v;
            }
        __syncthreads();
        dwl::sweeps(T, H, X0, R, lane, live);
    }
    // the small columns: the identity's for A^-1, then a right side of A f = g for every x0
    const int nid = lambda != nullptr ? m : 0, ncs = nid + R;
    if (live)
        for (int u = lane; u < ncs * m; u += L) {
            const int c = u / m, i = u - m * c;
            S[c * AS + i] = c < nid ? (i == c ? 1.0f : 0.0f)
                                    : dwc::g_word(T, E, gamma != nullptr ? gamma + env * m : nullptr, X0 + (c - nid) * NV, i);
        }
    __syncthreads();
    for (int j = 0; j < m - 1; ++j) {
        if (live)
            for (int u = lane; u < ncs * m; u += L) {
                const int c = u / m, i = u - m * c;
                if (i > j) dwc::sfwd_one(A, S + c * AS, j, i);
            }
        __syncthreads();
    }
    if (live)
        for (int u = lane; u < ncs * m; u += L) {
            const int c = u / m;
            dwc::sscale_one(A, S + c * AS, u - m * c);
        }
    __syncthreads();
    for (int j = m - 1; j >= 1; --j) {
        if (live)
            for (int u = lane; u < ncs * m; u += L) {
                const int c = u / m, i = u - m * c;
                if (i < j) dwc::sback_one(A, S + c * AS, j, i);
            }
        __syncthreads();
    }
    if (live) {
        if (lambda != nullptr)
            for (int i = lane; i < m * m; i += L) {
                const int r = i / m;
                lambda[env * m * m + i] = dwc::mirror_word(S, r, i - m * r);
            }
        if (force != nullptr)
            for (int u = lane; u < R * m; u += L) {
                const int c = u / m;
                force[env * R * m + u] = S[(nid + c) * AS + u - m * c];
            }
        if (accel != nullptr)
            for (int u = lane; u < R * NV; u += L) {
                const int c = u / NV;
                accel[env * R * NV + u] = dwc::accel_word(E, X0 + c * NV, S + (nid + c) * AS, m, u - NV * c);
            }
    }
}

}  // namespace

extern "C" {

int dwc_abi_version(void) { return DWC_ABI_VERSION; }
const char *dwc_last_error(void) { return s_err.s; }

int dwc_pack_table(const DwjModel *m, const DwcContacts *contacts, uint32_t *table_host) {
    return dwc::pack(m, contacts, table_host, s_err.s, sizeof(s_err.s));
}

int dwc_solve(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
              const float *dof_armature, int32_t vel_at_com, const float *rhs, int32_t nrhs, const float *sub, const float *gamma, float *jc,
              float *jdnu, float *minv_jt, float *lambda_inv, float *lambda, float *accel, float *force, void *stream) {
    if (num_envs < 1 || num_envs > 0x7fffffff / (MAXM * NV) - G) return s_err.fail("dwc_solve: num_envs must be in [1, 2^31 / 936 - 3)");
    if (!table || !root_states || !dof_state) return s_err.fail("dwc_solve: a buffer is missing");
    if ((reinterpret_cast<uintptr_t>(table) & 15u) != 0u) return s_err.fail("dwc_solve: the table must be 16-byte aligned");
    if (rhs && !accel && !force) return s_err.fail("dwc_solve: rhs needs accel or force");
    if ((accel || force) && !rhs) return s_err.fail("dwc_solve: accel and force need rhs");
    if (sub && !rhs) return s_err.fail("dwc_solve: sub needs rhs");
    if (gamma && !rhs) return s_err.fail("dwc_solve: gamma needs rhs");
    if (rhs && (nrhs < 1 || nrhs > DWC_MAX_RHS)) return s_err.fail("dwc_solve: nrhs must be in 1..DWC_MAX_RHS = 8");
    if (!jc && !jdnu && !minv_jt && !lambda_inv && !lambda && !accel && !force) return s_err.fail("dwc_solve: no output: nothing to compute");
    hipLaunchKernelGGL(dwc_k_solve, dim3(dwc::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs,
                       reinterpret_cast<const uint4 *>(table), root_states, dof_state, mass_scale, dof_armature, (int)(vel_at_com != 0), rhs,
                       (int)(rhs ? nrhs : 0), sub, gamma, jc, jdnu, minv_jt, lambda_inv, lambda, accel, force);
    return s_err.launched("dwc_solve");
}

}  // extern "C"
