// dw_forward_dynamics.hip -- the kernel of the forward dynamics (include/dyros_forward_dynamics.h).  The per-env
// arithmetic is dw_factor.h's and dw_jacobian.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds
// round alike.
// dwl_k_solve's front end is dwj_k_mass_matrix's: a workgroup of 256 lanes takes DWL_GROUP = 4 envs, a wave each; the model table and the envs'
// input rows come into LDS with consecutive lanes on consecutive words; a lane per (env, root-to-leaf path) walks the chain; a lane per (env,
// record) forms its inertia; a lane per (env, moving body) sums its subtree.  Then, per env over its 64 lanes: the 396 pattern words of M go
// into the env's store through dwj::mm_word; rows 38 down to 1 are eliminated in place, a row's at most 136 updates spread over the lanes
// (numbered s << 4 | t: four to a lane, all read before all written) with a barrier between rows; the multipliers are divided out in one pass; the factor is
// written; the right-hand sides -- the identity's columns for M^-1, then the caller's -- are solved dwl::CAP = 24 at a time in the LDS that
// the front end has left free: rows 38 down to 1 of L'^-1, the division by D, columns 0 up to 37 of L^-1, every step's independent updates
// (columns times the step's pattern words) spread over the lanes with a barrier between steps; then they are written.  An env's store is
// 5.5 KB, a workgroup's LDS 32 KB: five workgroups, 20 waves, share a CU's 160 KB.
// The loads are dw_group.h's; the inertia stage, the forming of H, the elimination and the sweeps are dw_factor_wave.h's, which dwc_k_solve
// (dw_contact_dynamics.hip) runs too: the two kernels factor M to the same bits because they run the same code.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "dw_factor_wave.h"
#include "dw_group.h"

namespace {

grp::Err s_err;

constexpr int G = DWL_GROUP, L = DWL_LANES, TPB = DWL_GROUP * DWL_LANES;
constexpr int IN_ROOT = dwb::IN_ROOT, IN_DOF = dwb::IN_DOF, NV = dwl::NV, NB = dwl::NB, ND = DWL_NUM_DOF, MMW = dwl::MMW;
static_assert(L == dwl::L && TPB % 64 == 0 && G * DWB_MAX_LEAVES <= 64, "a wave per env, the paths of a group in one wave");
static_assert(G * dwj::NI <= TPB && G * dwj::NM <= TPB, "a lane per record, a lane per moving body");
static_assert(dwl::CAP <= L && dwl::CAP * NV <= dwl::E_H, "a lane per column, the columns inside the front end's store");
static_assert((DWL_TABLE_WORDS + G * (IN_ROOT + IN_DOF + NB + ND + dwl::ENV)) * 4 <= 64 * 1024, "static LDS");

__global__ __launch_bounds__(TPB) void dwl_k_solve(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                   const float *__restrict__ dof_state, const float *__restrict__ mass_scale,
                                                   const float *__restrict__ dof_armature, int vel_at_com, const float *__restrict__ rhs, int nrhs,
                                                   const float *__restrict__ sub, float *__restrict__ x, float *__restrict__ factor,
                                                   float *__restrict__ minv) {
    __shared__ uint4 s_tab4[DWL_TABLE_WORDS / 4];
    __shared__ float s_root[G * IN_ROOT];
    __shared__ float s_dof[G * IN_DOF];
    __shared__ float s_ms[G * NB];
    __shared__ float s_arm[G * ND];
    __shared__ float s_env[G * dwl::ENV];
    const int t = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = n - e0 < G ? n - e0 : G;          // envs of this workgroup (the last one may hold fewer)
    const bool has_ms = mass_scale != nullptr, has_arm = dof_armature != nullptr;
    grp::load_table<TPB, DWL_TABLE_WORDS>(table, t, s_tab4);
    grp::load_rows<TPB>(root_states, e0, ne, IN_ROOT, t, s_root);
    grp::load_rows<TPB>(dof_state, e0, ne, IN_DOF, t, s_dof);
    if (has_ms) grp::load_rows<TPB>(mass_scale, e0, ne, NB, t, s_ms);
    if (has_arm) grp::load_rows<TPB>(dof_armature, e0, ne, ND, t, s_arm);
    __syncthreads();
    const dwb::Tab T{reinterpret_cast<const uint32_t *>(s_tab4)};
    const int nleaf = T.nleaf();
    if (nleaf > 0 && t < ne * nleaf) {
        const int ce = t / nleaf;
        dwj::walk_path(T, t - nleaf * ce, s_root + ce * IN_ROOT, s_dof + ce * IN_DOF, vel_at_com, s_env + ce * dwl::ENV);
    }
    __syncthreads();
    dwl::inertia<dwl::ENV>(T, s_env, has_ms, s_ms, ne, t);
    // from here on a wave per env; the barriers are the workgroup's, the row loop is the same for every env
    const int e = t / L, lane = t - e * L;
    const bool live = e < ne;
    float *E = s_env + (live ? e : 0) * dwl::ENV, *H = E + dwl::E_H;
    dwl::form(T, E, H, has_arm ? s_arm + e * ND : nullptr, lane, live);
    dwl::eliminate(T, H, lane, live);
    const size_t env = (size_t)(e0 + e);
    if (live && factor != nullptr) {
        float *out = factor + env * MMW;
        for (int i = lane; i < MMW; i += L) {
            const int r = i / NV;
            out[i] = dwl::factor_word(T, H, r, i - NV * r);
        }
    }
    // the columns: the identity's 39 when M^-1 is asked for, then the caller's right-hand sides; CAP of them at a time in the front end's store
    const int nid = minv != nullptr ? NV : 0, ncol = nid + (x != nullptr ? nrhs : 0);
    for (int c0 = 0; c0 < ncol; c0 += dwl::CAP) {
        const int nc = ncol - c0 < dwl::CAP ? ncol - c0 : dwl::CAP;
        if (live) {
            for (int i = lane; i < nc * NV; i += L) {
                const int c = i / NV, k = i - NV * c, col = c0 + c;
                float v;
                if (col < nid) {
                    v = k == col ? 1.0f : 0.0f;
                } else {
                    v = rhs[(env * nrhs + (col - nid)) * NV + k];
                    v -= sub != nullptr ? sub[env * NV + k] : 0.0f;
                }
                E[i] = v;
            }
        }
        __syncthreads();
        dwl::sweeps(T, H, E, nc, lane, live);
        if (live) {
            if (c0 < nid) {
                float *out = minv + env * MMW;
                for (int i = lane; i < MMW; i += L) {
                    const int r = i / NV;
                    float v;
                    if (dwl::minv_word(E, c0, (nid - c0 < nc ? nid - c0 : nc), r, i - NV * r, &v)) out[i] = v;
                }
            }
            if (c0 + nc > nid) {
                // columns max(c0, nid) .. c0 + nc - 1 are right-hand sides max(c0, nid) - nid ..: one contiguous run of x
                const int first = c0 > nid ? c0 : nid;
                float *out = x + (env * nrhs + (first - nid)) * NV;
                const float *src = E + (first - c0) * NV;
                for (int i = lane; i < (c0 + nc - first) * NV; i += L) out[i] = src[i];
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

int dwl_abi_version(void) { return DWL_ABI_VERSION; }
const char *dwl_last_error(void) { return s_err.s; }

int dwl_pack_table(const DwjModel *m, uint32_t *table_host) { return dwl::pack(m, table_host, s_err.s, sizeof(s_err.s)); }

int dwl_solve(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
              const float *dof_armature, int32_t vel_at_com, const float *rhs, int32_t nrhs, const float *sub, float *x, float *factor,
              float *minv, void *stream) {
    if (num_envs < 1 || num_envs > 0x7fffffff / MMW - G) return s_err.fail("dwl_solve: num_envs must be in [1, 2^31 / 1521 - 4)");
    if (!table || !root_states || !dof_state) return s_err.fail("dwl_solve: a buffer is missing");
    if ((reinterpret_cast<uintptr_t>(table) & 15u) != 0u) return s_err.fail("dwl_solve: the table must be 16-byte aligned");
    if (rhs && !x) return s_err.fail("dwl_solve: rhs needs x");
    if (x && !rhs) return s_err.fail("dwl_solve: x needs rhs");
    if (sub && !rhs) return s_err.fail("dwl_solve: sub needs rhs");
    if (rhs && (nrhs < 1 || nrhs > DWL_MAX_RHS)) return s_err.fail("dwl_solve: nrhs must be in 1..DWL_MAX_RHS = 8");
    if (!x && !factor && !minv) return s_err.fail("dwl_solve: no output: nothing to compute");
    hipLaunchKernelGGL(dwl_k_solve, dim3(dwl::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs,
                       reinterpret_cast<const uint4 *>(table), root_states, dof_state, mass_scale, dof_armature, (int)(vel_at_com != 0), rhs,
                       (int)(rhs ? nrhs : 0), sub, x, factor, minv);
    return s_err.launched("dwl_solve");
}

}  // extern "C"
