// dw_inverse_kinematics.hip -- the kernel of the inverse kinematics (include/dyros_inverse_kinematics.h), dwq_k_solve,
// and the ABI's entry points.  The per-env arithmetic is dw_inverse_kinematics.h's on top of dw_jacobian.h and dw_contact.h, shared with a
// g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
// A workgroup of 256 lanes takes DWQ_GROUP = 4 envs.  The table, the envs' root and dof_state rows and their targets come into LDS; q0, when
// given, overwrites the positions of the dof_state rows there, and from then on those rows and the root rows ARE the iterate: the walk reads
// them unchanged.  Every pass of the loop: a lane per (env, path) walks the chain (first wave); then a wave per env: a lane per target forms
// its point, a lane per row its error word, lane 0 the env's status; a lane per word of J, then of A's folded triangle (and of the right
// side); the columns of the factor over the square still to update, the two sweeps with a lane per row; a lane per column of dnu; a lane per
// joint (and lane 33 for the base) for the update.  One more walk after the loop gives residual, err and converged.
// The barriers are the workgroup's and stand outside divergent control flow: the loop runs the table's trip count in every lane, m comes
// from the table, `live` guards what every env does and `mv` (live, not done, not dead) the update; no lane leaves before the last barrier.
// An env's store is 1979 words; with its input rows 8.3 KB, a workgroup 38.3 KB: four workgroups -- 16 envs -- share a CU's 160 KB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include "dw_inverse_kinematics.h"
#include "dw_group.h"

namespace {

grp::Err s_err;

constexpr int G = DWQ_GROUP, L = DWQ_LANES, TPB = DWQ_GROUP * DWQ_LANES;
constexpr int IN_ROOT = dwb::IN_ROOT, IN_DOF = dwb::IN_DOF, NV = dwq::NV, ND = dwq::ND, MAXM = dwq::MAXM, MAXK = dwq::MAXK, TW = dwq::TW, ENV = dwq::ENV;
static_assert(L == 64 && G * DWB_MAX_LEAVES <= L, "a wave per env, the paths of a group in the first wave");
static_assert(MAXK <= L && MAXM <= L && NV <= L && ND + 1 <= L, "a lane per target, per row, per column of dnu, per joint and one for the base");
static_assert((DWQ_TABLE_WORDS + G * (IN_ROOT + IN_DOF + MAXK * TW + ENV)) * 4 <= 160 * 1024 / 4, "four workgroups to a CU");

__global__ __launch_bounds__(TPB) void dwq_k_solve(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                   const float *__restrict__ dof_state, const float *__restrict__ q0,
                                                   const float *__restrict__ targets, float *__restrict__ q, float *__restrict__ root_out,
                                                   float *__restrict__ residual, float *__restrict__ err, int32_t *__restrict__ iters,
                                                   uint8_t *__restrict__ converged) {
    __shared__ uint4 s_tab4[DWQ_TABLE_WORDS / 4];
    __shared__ float s_root[G * IN_ROOT];
    __shared__ float s_dof[G * IN_DOF];
    __shared__ float s_tgt[G * MAXK * TW];
    __shared__ float s_env[G * ENV];
    const int t = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = n - e0 < G ? n - e0 : G;          // envs of this workgroup (the last one may hold fewer)
    grp::load_table<TPB, DWQ_TABLE_WORDS>(table, t, s_tab4);
    grp::load_rows<TPB>(root_states, e0, ne, IN_ROOT, t, s_root);
    grp::load_rows<TPB>(dof_state, e0, ne, IN_DOF, t, s_dof);
    __syncthreads();
    const dwb::Tab T{reinterpret_cast<const uint32_t *>(s_tab4)};
    const int nleaf = T.nleaf(), K = dwq::count(T), m = 6 * K, I = dwq::iterations(T);
    const bool free_base = dwq::flag(T, DWQ_F_FREE_BASE);
    // the targets (K comes from the table), q0 over the rows' positions, the state words
    for (int i = t; i < ne * K * TW; i += TPB) {
        const int ce = i / (K * TW);
        s_tgt[ce * MAXK * TW + (i - ce * K * TW)] = targets[(size_t)e0 * (K * TW) + i];
    }
    if (q0 != nullptr)
        for (int i = t; i < ne * ND; i += TPB) {
            const int ce = i / ND;
            s_dof[ce * IN_DOF + 2 * (i - ce * ND)] = q0[(size_t)e0 * ND + i];
        }
    if (t < G * 3) s_env[(t / 3) * ENV + dwq::E_DEAD + (t % 3)] = 0.0f;
    __syncthreads();
    // from the walk on a wave per env
    const int e = t / L, lane = t - e * L;
    const bool live = e < ne;
    const int se = live ? e : 0;
    const size_t env = (size_t)(e0 + se);
    float *E = s_env + se * ENV, *root = s_root + se * IN_ROOT, *dof = s_dof + se * IN_DOF;
    const float *tgt = s_tgt + se * MAXK * TW;
    // the walk, the points, the error rows, the status: three barriers, every lane passes them
    auto look = [&]() {
        if (nleaf > 0 && t < ne * nleaf) {
            const int ce = t / nleaf;
            dwj::walk_path(T, t - nleaf * ce, s_root + ce * IN_ROOT, s_dof + ce * IN_DOF, 0, s_env + ce * ENV + dwj::E_KS);
        }
        __syncthreads();
        if (live && lane < K) dwq::point(T, E, lane);
        __syncthreads();
        if (live && lane < m) dwq::err_row(T, E, root, tgt, lane);
        __syncthreads();
        if (live && lane == 0) dwq::status(T, E, tgt, K);
        __syncthreads();
    };
    for (int it = 0; it < I; ++it) {
        look();
        const bool mv = live && dwq::moving(E);
        if (mv)
            for (int i = lane; i < m * NV; i += L) {
                const int r = i / NV;
                dwq::j_word(T, E, r, i - NV * r);
            }
        __syncthreads();
        if (mv) {
            for (int u = lane; u < m / 2 * (m + 1); u += L) dwq::a_word(T, E, m, u);
            if (lane < m) E[dwq::E_Y + lane] = E[dwq::E_ERR + lane];
        }
        __syncthreads();
        float *A = E + dwq::E_A, *Y = E + dwq::E_Y;
        // A = L D L': column j's updates read column j and write the square to its right and below
        for (int j = 0; j < m - 1; ++j) {
            const int w = m - 1 - j;
            if (mv)
                for (int x = lane; x < w * w; x += L) {
                    const int i = j + 1 + x / w, k = j + 1 + (x - w * (x / w));
                    if (k <= i) dwc::ldl_one(A, j, i, k);
                }
            __syncthreads();
        }
        if (mv)
            for (int x = lane; x < m * m; x += L) {
                const int i = x / m, j = x - m * i;
                if (j < i) dwc::ldl_scale(A, i, j);
            }
        __syncthreads();
        for (int j = 0; j < m - 1; ++j) {
            if (mv && lane < m && lane > j) dwc::sfwd_one(A, Y, j, lane);
            __syncthreads();
        }
        if (mv && lane < m) dwc::sscale_one(A, Y, lane);
        __syncthreads();
        for (int j = m - 1; j >= 1; --j) {
            if (mv && lane < j) dwc::sback_one(A, Y, j, lane);
            __syncthreads();
        }
        if (mv && lane < NV) dwq::dv_word(E, m, lane);
        __syncthreads();
        if (mv) {
            const float s = dwq::step_scale(T, E);
            if (lane < ND) dwq::update_joint(T, E, dof, lane, s);
            else if (lane == ND && free_base) dwq::update_base(E, root, s);
            else if (lane == ND + 1) E[dwq::E_ITERS] += 1.0f;
        }
        __syncthreads();
    }
    look();
    if (!live) return;          // (after the last barrier)
    const bool dead = E[dwq::E_DEAD] != 0.0f;
    const float nan = __int_as_float(0x7fc00000);
    if (q != nullptr && lane < ND) q[env * ND + lane] = dead ? nan : dof[2 * lane];
    if (root_out != nullptr && lane < 7) {
        // a fixed base: the caller's bits (the LDS row was never written); a free one: the iterate
        root_out[env * 7 + lane] = dead ? nan : root[lane];
    }
    if (residual != nullptr && lane < m) residual[env * m + lane] = dead ? nan : E[dwq::E_ERR + lane];
    if (err != nullptr && lane < 2) err[env * 2 + lane] = dead ? nan : dwq::err_max(T, E, K, lane);
    if (lane == 0) {
        if (iters != nullptr) iters[env] = dead ? 0 : (int32_t)E[dwq::E_ITERS];
        if (converged != nullptr) converged[env] = E[dwq::E_DONE] != 0.0f ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int dwq_abi_version(void) { return DWQ_ABI_VERSION; }
const char *dwq_last_error(void) { return s_err.s; }

int dwq_pack_table(const DwjModel *m, const DwcContacts *targets, const uint8_t *row_mask, const float *weights, const uint8_t *dof_mask,
                   const float *dof_lower, const float *dof_upper, const DwqParams *params, uint32_t *table_host) {
    return dwq::pack(m, targets, row_mask, weights, dof_mask, dof_lower, dof_upper, params, table_host, s_err.s, sizeof(s_err.s));
}

int dwq_solve(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *q0, const float *targets,
              float *q, float *root_out, float *residual, float *err, int32_t *iters, uint8_t *converged, void *stream) {
    const char *who = "dwq_solve";
    if (num_envs < 1 || num_envs > 0x7fffffff / IN_DOF - G) return s_err.fail(who, "num_envs must be in [1, 2^31 / 66 - 4)");
    if (!table || !root_states || !dof_state || !targets) return s_err.fail(who, "a buffer is missing");
    if ((reinterpret_cast<uintptr_t>(table) & 15u) != 0u) return s_err.fail(who, "the table must be 16-byte aligned");
    if (!q && !root_out && !residual && !err && !iters && !converged) return s_err.fail(who, "no output: nothing to compute");
    hipLaunchKernelGGL(dwq_k_solve, dim3(dwq::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs, reinterpret_cast<const uint4 *>(table),
                       root_states, dof_state, q0, targets, q, root_out, residual, err, iters, converged);
    return s_err.launched("dwq_solve");
}

}  // extern "C"
