// dw_contact_inverse.hip -- the kernels of the contact inverse dynamics (include/dyros_contact_inverse_dynamics.h) and of
// the stance inverse dynamics (include/dyros_stance_inverse_dynamics.h; section 28): one body, solve<STANCE>, under the two names dwi_k_solve
// and dwk_k_solve, and both ABIs' entry points.  The per-env arithmetic is dw_contact_inverse.h's and dw_stance_inverse.h's on top of
// dw_dynamics.h and dw_jacobian.h, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
// The body is dwn_k_inverse_dynamics with a tail: a workgroup of 256 lanes takes DWI_GROUP = 4 envs; the table and the envs' input rows
// come into LDS; a lane per (env, path) walks the chain with the caller's nu_dot; a lane per (env, record) leaves the record's wrench while,
// in the last wave, a lane per (env, contact) forms the contact's point and J_c a + Jd_c nu; a lane per (env, moving body) sums its subtree
// to its word of r.  From there on a wave per env: G's 21 words and the six words of the right side with a lane each, the five columns of
// the factor and the two sweeps with a barrier between steps, f with a lane per row, tau_joint with a lane per joint.  The barriers are the
// workgroup's and stand outside divergent control flow: every loop bound comes from the table or is a constant, `live` guards what every env
// does and `act` the sums, the factor and the sweeps.  STANCE is a compile-time switch, the same for every lane.
// Without it (dwi_k_solve) every contact carries load: the mask is all K bits and act is live.  With it (dwk_k_solve) each env's stance comes
// into LDS as one mask word -- the four envs of a workgroup differ in stance -- act is live with a stance that is not empty, and beside
// tau_joint's lanes margins, base_residual and feasible are formed straight into global memory: six lanes, one lane, a lane per (contact,
// word).  An env's store is dw_dynamics.h's 7.7 KB and 108 words; a workgroup's LDS stays below a quarter of a CU's 160 KB, as dwn's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "dw_stance_inverse.h"
#include "dw_group.h"

namespace {

grp::Err s_err_i, s_err_k;          // (the error is per ABI)

constexpr int G = DWI_GROUP, L = DWI_LANES, TPB = DWI_GROUP * DWI_LANES;
constexpr int IN_ROOT = dwb::IN_ROOT, IN_DOF = dwb::IN_DOF, NV = dwi::NV, NB = dwi::NB, ND = dwi::ND, GN = dwi::GN, MAXM = dwi::MAXM, MW = dwk::MW;
static_assert(L == 64 && G * DWB_MAX_LEAVES <= 64, "a wave per env, the paths of a group in one wave");
static_assert(G * dwn::NI <= TPB - L && G * dwi::MAXK + G <= L && G * dwn::NM <= TPB, "the records leave the last wave to the contacts and the masks; a lane per moving body");
static_assert(dwi::GW + GN <= L && GN * GN <= L && MAXM <= L && NV <= L, "a lane per word of G and of its right side, per row, per joint");
static_assert(ND + GN + 1 + dwk::MAXK * MW <= L, "a lane per joint, per base row, for feasible and per margin, side by side");
static_assert((DWK_TABLE_WORDS + G * (IN_ROOT + IN_DOF + NB + ND + NV + dwi::ENV + 1)) * 4 <= 160 * 1024 / 4, "four workgroups to a CU, as dwn");

template <bool STANCE>
__device__ __forceinline__ void solve(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states, const float *__restrict__ dof_state,
                                      const float *__restrict__ mass_scale, const float *__restrict__ dof_armature, float gx, float gy, float gz,
                                      const float *__restrict__ accel, const float *__restrict__ force_ref, const uint8_t *__restrict__ stance,
                                      int vel_at_com, float *__restrict__ tau_joint, float *__restrict__ force, float *__restrict__ contact_accel,
                                      float *__restrict__ tau_full, float *__restrict__ base_residual, float *__restrict__ margins,
                                      uint8_t *__restrict__ feasible) {
    constexpr int TABLE_WORDS = STANCE ? DWK_TABLE_WORDS : DWI_TABLE_WORDS;
    __shared__ uint4 s_tab4[TABLE_WORDS / 4];
    __shared__ float s_root[G * IN_ROOT];
    __shared__ float s_dof[G * IN_DOF];
    __shared__ float s_ms[G * NB];
    __shared__ float s_arm[G * ND];
    __shared__ float s_acc[G * NV];
    __shared__ float s_env[G * dwi::ENV];
    __shared__ uint32_t s_mask[G];          // (STANCE only: never touched, and so not allocated, without it)
    const int t = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = n - e0 < G ? n - e0 : G;          // envs of this workgroup (the last one may hold fewer)
    // (dwi_k_solve passes NULL for stance and for the last three outputs: their tests fold away there)
    const bool need_f = force != nullptr || tau_joint != nullptr || base_residual != nullptr || margins != nullptr || feasible != nullptr;
    const bool need_r = need_f || tau_full != nullptr;
    const int what = need_r ? dwn::W_TAU : 0;
    const bool has_acc = accel != nullptr, has_ms = mass_scale != nullptr, has_arm = has_acc && dof_armature != nullptr;
    grp::load_table<TPB, TABLE_WORDS>(table, t, s_tab4);
    grp::load_rows<TPB>(root_states, e0, ne, IN_ROOT, t, s_root);
    grp::load_rows<TPB>(dof_state, e0, ne, IN_DOF, t, s_dof);
    if (has_ms && need_r) grp::load_rows<TPB>(mass_scale, e0, ne, NB, t, s_ms);
    if (has_arm && need_r) grp::load_rows<TPB>(dof_armature, e0, ne, ND, t, s_arm);
    if (has_acc) grp::load_rows<TPB>(accel, e0, ne, NV, t, s_acc);
    __syncthreads();
    const dwb::Tab T{reinterpret_cast<const uint32_t *>(s_tab4)};
    const float g[3] = {gx, gy, gz};
    const int nleaf = T.nleaf(), K = dwi::count(T), m = 6 * K;
    // the envs' stances as mask words: the last wave's lanes past the contacts' take them
    const int tc = t - (TPB - L);
    if constexpr (STANCE)
        if (tc >= L - G && tc - (L - G) < ne) {
            const int ce = tc - (L - G);
            s_mask[ce] = dwk::mask_of(stance != nullptr ? stance + (size_t)(e0 + ce) * K : nullptr, K);
        }
    // a NULL nu_dot is zero: the walk then leaves the nu_dot = 0 words in the caller's slots as well
    if (nleaf > 0 && t < ne * nleaf) {
        const int ce = t / nleaf;
        dwn::walk_path(T, t - nleaf * ce, s_root + ce * IN_ROOT, s_dof + ce * IN_DOF, has_acc ? s_acc + ce * NV : nullptr, vel_at_com,
                       s_env + ce * dwi::ENV);
    }
    __syncthreads();
    // f_ref into the envs' stores (zeros when the caller has none: the same arithmetic, the same bits); an inactive row's word is not read
    if (need_f)
        for (int i = t; i < ne * m; i += TPB) {
            const int ce = i / m, r = i - m * ce;
            s_env[ce * dwi::ENV + dwi::E_FR + r] = force_ref != nullptr && (!STANCE || dwi::on(s_mask[ce], r / 6)) ? force_ref[(size_t)e0 * m + i] : 0.0f;
        }
    if (need_r && t < ne * dwn::NI) {
        const int ce = t / dwn::NI;
        dwn::record(T, s_env + ce * dwi::ENV, has_ms ? s_ms + ce * NB : nullptr, g, what, t - ce * dwn::NI);
    }
    // (the last wave holds no record: its first lanes take the contacts)
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
    uint32_t mask = dwi::full(K);
    if constexpr (STANCE) mask = live ? s_mask[e] : 0u;
    const bool act = live && (!STANCE || mask != 0u);
    if (live) {
        if (contact_accel != nullptr && lane < m) contact_accel[env * m + lane] = E[dwi::E_CA + lane];
        if (tau_full != nullptr && lane < NV) tau_full[env * NV + lane] = E[dwi::E_TAU + lane];
    }
    if (!need_f) return;          // (every lane alike)
    if (act) {
        if (lane < dwi::GW) dwi::g_word(T, E, K, mask, lane);
        else if (lane < dwi::GW + GN) dwi::y_word(T, E, K, mask, lane - dwi::GW);
    }
    __syncthreads();
    // G = L D L': column j's updates read column j and write to its right
    for (int j = 0; j < GN - 1; ++j) {
        if (act && lane < GN * GN) {
            const int i = lane / GN, k = lane - GN * i;
            if (k > j && k <= i) dwi::ldl_one(Gm, j, i, k);
        }
        __syncthreads();
    }
    if (act && lane < GN * GN) {
        const int i = lane / GN, j = lane - GN * i;
        if (j < i) dwi::ldl_scale(Gm, i, j);
    }
    __syncthreads();
    for (int j = 0; j < GN - 1; ++j) {
        if (act && lane < GN && lane > j) dwi::sfwd_one(Gm, Y, j, lane);
        __syncthreads();
    }
    if (act && lane < GN) dwi::sscale_one(Gm, Y, lane);
    __syncthreads();
    for (int j = GN - 1; j >= 1; --j) {
        if (act && lane < j) dwi::sback_one(Gm, Y, j, lane);
        __syncthreads();
    }
    if (live && lane < m) {
        dwi::f_word(T, E, mask, lane);
        if (force != nullptr) force[env * m + lane] = E[dwi::E_F + lane];
    }
    if (tau_joint == nullptr && base_residual == nullptr && margins == nullptr && feasible == nullptr) return;
    __syncthreads();
    if (!live) return;
    // a lane per joint; under STANCE then six lanes, one lane, and a lane per (contact, word)
    if (lane < ND) {
        if (tau_joint != nullptr) tau_joint[env * ND + lane] = dwi::tauj_word(T, E, K, mask, lane);
    } else if constexpr (STANCE) {
        if (lane < ND + GN) {
            if (base_residual != nullptr) base_residual[env * GN + (lane - ND)] = dwk::base_word(T, E, K, mask, lane - ND);
        } else if (lane == ND + GN) {
            if (feasible != nullptr) feasible[env] = dwk::feasible_of(T, E, K, mask);
        } else if (lane - (ND + GN + 1) < K * MW) {
            if (margins != nullptr) {
                const int u = lane - (ND + GN + 1), i = u / MW;
                float o[4];
                dwk::margins4(T, E, mask, i, o);
                const int w = u - MW * i;
                margins[env * (size_t)(K * MW) + u] = w == 0 ? o[0] : (w == 1 ? o[1] : (w == 2 ? o[2] : o[3]));
            }
        }
    }
}

__global__ __launch_bounds__(TPB) void dwi_k_solve(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                   const float *__restrict__ dof_state, const float *__restrict__ mass_scale,
                                                   const float *__restrict__ dof_armature, float gx, float gy, float gz,
                                                   const float *__restrict__ accel, const float *__restrict__ force_ref, int vel_at_com,
                                                   float *__restrict__ tau_joint, float *__restrict__ force, float *__restrict__ contact_accel,
                                                   float *__restrict__ tau_full) {
    solve<false>(n, table, root_states, dof_state, mass_scale, dof_armature, gx, gy, gz, accel, force_ref, nullptr, vel_at_com, tau_joint, force,
                 contact_accel, tau_full, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(TPB) void dwk_k_solve(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                   const float *__restrict__ dof_state, const float *__restrict__ mass_scale,
                                                   const float *__restrict__ dof_armature, float gx, float gy, float gz,
                                                   const float *__restrict__ accel, const float *__restrict__ force_ref,
                                                   const uint8_t *__restrict__ stance, int vel_at_com, float *__restrict__ tau_joint,
                                                   float *__restrict__ force, float *__restrict__ contact_accel, float *__restrict__ tau_full,
                                                   float *__restrict__ base_residual, float *__restrict__ margins, uint8_t *__restrict__ feasible) {
    solve<true>(n, table, root_states, dof_state, mass_scale, dof_armature, gx, gy, gz, accel, force_ref, stance, vel_at_com, tau_joint, force,
                contact_accel, tau_full, base_residual, margins, feasible);
}

// the refusals both entry points share, under the caller's name `who`, then the launch: the kernel's arguments after gz are `rest`
template <class Kernel, class... Rest>
int launch(grp::Err &err, const char *who, Kernel kernel, bool any_output, void *stream, int32_t num_envs, const uint32_t *table, const float *root_states,
           const float *dof_state, const float *mass_scale, const float *dof_armature, float gx, float gy, float gz, Rest... rest) {
    if (num_envs < 1 || num_envs > 0x7fffffff / (IN_DOF + NV) - G) return err.fail(who, "num_envs must be in [1, 2^31 / 105 - 4)");
    if (!table || !root_states || !dof_state) return err.fail(who, "a buffer is missing");
    if ((reinterpret_cast<uintptr_t>(table) & 15u) != 0u) return err.fail(who, "the table must be 16-byte aligned");
    if (!any_output) return err.fail(who, "no output: nothing to compute");
    if (!isfinite(gx) || !isfinite(gy) || !isfinite(gz)) return err.fail(who, "the gravity vector is not finite");
    hipLaunchKernelGGL(kernel, dim3(dwn::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs, reinterpret_cast<const uint4 *>(table),
                       root_states, dof_state, mass_scale, dof_armature, gx, gy, gz, rest...);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    char where[32];
    snprintf(where, sizeof(where), "%s: launch", who);
    return err.fail_hip(where, e);
}

}  // namespace

extern "C" {

int dwi_abi_version(void) { return DWI_ABI_VERSION; }
const char *dwi_last_error(void) { return s_err_i.s; }

int dwi_pack_table(const DwjModel *m, const DwcContacts *contacts, const float *weights, uint32_t *table_host) {
    return dwi::pack(m, contacts, weights, table_host, s_err_i.s, sizeof(s_err_i.s));
}

int dwi_solve(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
              const float *dof_armature, float gx, float gy, float gz, const float *accel, const float *force_ref, int32_t vel_at_com,
              float *tau_joint, float *force, float *contact_accel, float *tau_full, void *stream) {
    return launch(s_err_i, "dwi_solve", dwi_k_solve, tau_joint || force || contact_accel || tau_full, stream, num_envs, table, root_states, dof_state,
                  mass_scale, dof_armature, gx, gy, gz, accel, force_ref, (int)(vel_at_com != 0), tau_joint, force, contact_accel, tau_full);
}

int dwk_abi_version(void) { return DWK_ABI_VERSION; }
const char *dwk_last_error(void) { return s_err_k.s; }

int dwk_pack_table(const DwjModel *m, const DwcContacts *contacts, const float *weights, const float *soles, float mu, uint32_t *table_host) {
    return dwk::pack(m, contacts, weights, soles, mu, table_host, s_err_k.s, sizeof(s_err_k.s));
}

int dwk_solve(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
              const float *dof_armature, float gx, float gy, float gz, const float *accel, const float *force_ref, const uint8_t *stance,
              int32_t vel_at_com, float *tau_joint, float *force, float *contact_accel, float *tau_full, float *base_residual, float *margins,
              uint8_t *feasible, void *stream) {
    return launch(s_err_k, "dwk_solve", dwk_k_solve, tau_joint || force || contact_accel || tau_full || base_residual || margins || feasible, stream,
                  num_envs, table, root_states, dof_state, mass_scale, dof_armature, gx, gy, gz, accel, force_ref, stance, (int)(vel_at_com != 0),
                  tau_joint, force, contact_accel, tau_full, base_residual, margins, feasible);
}

}  // extern "C"
