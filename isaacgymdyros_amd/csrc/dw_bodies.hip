// dw_bodies.hip -- the kernel of the rigid-body state tensor (include/dyros_bodies.h).  The per-env arithmetic is
// dw_bodies.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
//   dwb_k_refresh  one launch.  79 words are read and up to 38 * 13 + 7 = 501 written per env: a store stream.  A workgroup of 256 lanes takes
//                  DWB_GROUP = 16 envs, sixteen lanes each.  The model table and the envs' root rows, joint rows and mass scales (contiguous blocks) come into LDS
//                  with consecutive lanes on consecutive words.  A lane per (env, root-to-leaf path), packed into the first 80 lanes, then walks its
//                  path (two legs 6 deep, waist + arm 11 deep twice, waist + neck + head 5 deep) and leaves the moving bodies' states in LDS;
//                  an env's sixteen lanes sum strided shares of the inertial records and add them up with four shuffles.  Last, the
//                  group's contiguous [ne * nb * 13] block of `states` is written by consecutive lanes, 16 bytes per lane where `states` is
//                  16-byte aligned (a group's block then is too), every word formed from the LDS store on the way out; likewise [ne * 7] of
//                  `com`.  The subset path is the same code with another row list.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "dw_bodies.h"
#include "dw_group.h"

namespace {

grp::Err s_err;

constexpr int G = DWB_GROUP, TPB = DWB_GROUP * DWB_LANES;
static_assert(TPB % 64 == 0 && DWB_LANES == 16 && DWB_MAX_LEAVES <= DWB_LANES, "whole waves, sixteen lanes per env, room for a lane per path");
static_assert((G * dwb::IN_ROOT) % 4 == 0 && (G * DWB_ROW) % 4 == 0, "a group's blocks start on 16 bytes");
static_assert((DWB_TABLE_WORDS + G * (dwb::IN_ROOT + dwb::IN_DOF + dwb::NB + dwb::MVW + DWB_COM_WORDS) + dwb::NB) * 4 <= 64 * 1024, "static LDS");

struct Ids {
    unsigned char b[40];
};

__global__ __launch_bounds__(TPB) void dwb_k_refresh(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                     const float *__restrict__ dof_state, const float *__restrict__ mass_scale, Ids ids, int nb,
                                                     int vel_at_com, float *__restrict__ states, float *__restrict__ com) {
    __shared__ uint4 s_tab4[DWB_TABLE_WORDS / 4];
    __shared__ float s_root[G * dwb::IN_ROOT];
    __shared__ float s_dof[G * dwb::IN_DOF];
    __shared__ float s_ms[G * dwb::NB];
    __shared__ float s_mv[G * dwb::MVW];
    __shared__ float s_com[G * DWB_COM_WORDS];
    __shared__ int s_ids[dwb::NB];
    const int t = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = n - e0 < G ? n - e0 : G;          // envs of this workgroup (the last one may hold fewer)
    // ---- loads: consecutive lanes, consecutive words ----
    grp::load_table<TPB, DWB_TABLE_WORDS>(table, t, s_tab4);
    grp::load_rows<TPB>(root_states, e0, ne, dwb::IN_ROOT, t, s_root);
    grp::load_rows<TPB>(dof_state, e0, ne, dwb::IN_DOF, t, s_dof);
    if (mass_scale != nullptr && com != nullptr) grp::load_rows<TPB>(mass_scale, e0, ne, dwb::NB, t, s_ms);
    __syncthreads();
    const dwb::Tab T{reinterpret_cast<const uint32_t *>(s_tab4)};
    if (t < nb) s_ids[t] = dwb::row_of(T, ids.b[t] < dwb::NB ? ids.b[t] : dwb::NB - 1);          // (read after the barrier below)
    const int el = t / DWB_LANES, l = t - DWB_LANES * el;
    // ---- a lane per (env, path), packed into the first lanes: every wave that holds a path issues the whole 11-link stream, so the
    //      16 * 5 paths sit in two waves and the other two skip the phase ----
    const int nleaf = T.nleaf();
    if (nleaf > 0 && t < ne * nleaf) {
        const int ce = t / nleaf;
        dwb::walk_path(T, t - nleaf * ce, s_root + ce * dwb::IN_ROOT, s_dof + ce * dwb::IN_DOF, vel_at_com, s_mv + ce * dwb::MVW);
    }
    __syncthreads();
    // ---- centre of mass: a strided share of the records per lane, summed over the env's lanes ----
    if (com != nullptr) {
        if (el < ne) {
            float acc[DWB_COM_WORDS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            dwb::com_part(T, s_mv + el * dwb::MVW, mass_scale != nullptr ? s_ms + el * dwb::NB : nullptr, l, DWB_LANES, acc);
#pragma unroll
            for (int m = 1; m < DWB_LANES; m <<= 1) {
#pragma unroll
                for (int i = 0; i < DWB_COM_WORDS; ++i) acc[i] += __shfl_xor(acc[i], m, DWB_LANES);
            }
            if (l == 0) {
                float c7[DWB_COM_WORDS];
                dwb::com_finish(acc, s_root + el * dwb::IN_ROOT, c7);
#pragma unroll
                for (int i = 0; i < DWB_COM_WORDS; ++i) s_com[el * DWB_COM_WORDS + i] = c7[i];
            }
        }
        __syncthreads();
        float *dst = com + (size_t)e0 * DWB_COM_WORDS;
        for (int i = t; i < ne * DWB_COM_WORDS; i += TPB) dst[i] = s_com[i];
    }
    // ---- the group's rows: one contiguous block ----
    if (states != nullptr) {
        const int rw = nb * DWB_ROW, total = ne * rw;
        float *dst = states + (size_t)e0 * rw;
        auto word = [&](int e, int r) {
            const int k = r / DWB_ROW;
            return dwb::out_word(T, s_mv + e * dwb::MVW, s_root + e * dwb::IN_ROOT, s_ids[k], r - DWB_ROW * k, vel_at_com);
        };
        int done = 0;
        if ((reinterpret_cast<uintptr_t>(states) & 15u) == 0u) {
            const int nv = total / 4;
            for (int i4 = t; i4 < nv; i4 += TPB) {
                int e = (4 * i4) / rw, r = 4 * i4 - e * rw;
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = word(e, r);
                    if (++r == rw) { r = 0; ++e; }
                }
                reinterpret_cast<float4 *>(dst)[i4] = make_float4(v[0], v[1], v[2], v[3]);
            }
            done = 4 * nv;
        }
        for (int i = done + t; i < total; i += TPB) {
            const int e = i / rw;
            dst[i] = word(e, i - e * rw);
        }
    }
}

}  // namespace

extern "C" {

int dwb_abi_version(void) { return DWB_ABI_VERSION; }
const char *dwb_last_error(void) { return s_err.s; }

int dwb_pack_table(const DwbModel *m, uint32_t *table_host) { return dwb::pack(m, table_host, s_err.s, sizeof(s_err.s)); }

int dwb_refresh(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
                const int32_t *body_ids_host, int32_t nb, int32_t vel_at_com, float *states, float *com, void *stream) {
    if (num_envs < 1 || num_envs > 0x7fffffff / (DWB_NUM_BODIES * DWB_ROW) - G) return s_err.fail("dwb_refresh: num_envs must be in [1, 2^31 / 494 - 16)");
    if (!table || !root_states || !dof_state) return s_err.fail("dwb_refresh: a buffer is missing");
    if (!states && !com) return s_err.fail("dwb_refresh: states or com must be given");
    if ((reinterpret_cast<uintptr_t>(table) & 15u) != 0u) return s_err.fail("dwb_refresh: the table must be 16-byte aligned");
    Ids ids;
    if (body_ids_host == nullptr) {
        if (nb != 0 && nb != DWB_NUM_BODIES) return s_err.fail("dwb_refresh: without body ids nb must be 0 or 38");
        nb = DWB_NUM_BODIES;
        for (int k = 0; k < 40; ++k) ids.b[k] = (unsigned char)(k < DWB_NUM_BODIES ? k : 0);
    } else {
        if (nb < 1 || nb > DWB_NUM_BODIES) return s_err.fail("dwb_refresh: nb must be in 1..38");
        for (int k = 0; k < 40; ++k) ids.b[k] = 0;
        for (int k = 0; k < nb; ++k) {
            if (body_ids_host[k] < 0 || body_ids_host[k] >= DWB_NUM_BODIES) return s_err.fail("dwb_refresh: a body id is outside 0..37");
            ids.b[k] = (unsigned char)body_ids_host[k];
        }
    }
    hipLaunchKernelGGL(dwb_k_refresh, dim3(dwb::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs,
                       reinterpret_cast<const uint4 *>(table), root_states, dof_state, mass_scale, ids, (int)nb, (int)(vel_at_com != 0), states, com);
    return s_err.launched("dwb_refresh");
}

}  // extern "C"
