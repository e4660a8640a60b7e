// dw_height_scan.hip -- the kernel of the terrain height scan (include/dyros_height_scan.h).  The per-env arithmetic is
// dw_height_scan.h's, shared with a g++ build of the tests.  Built with -ffp-contract=off so that both builds round alike.
//   dwh_k_scan  one launch.  A workgroup of 256 lanes takes DWH_GROUP = 16 envs.  The table (the chain, the grid offsets, the probes) and the
//               envs' root and joint rows come into LDS with consecutive lanes on consecutive words.  Sixteen lanes per env check that its
//               inputs are finite and one of them forms its yaw pair, once.  With probes in the table, a lane per (env, walk) runs the chain
//               from the base down to a probe's carrier (the default, the eight sole corners: the two legs, 6 links each) and leaves the
//               carrier's pose in LDS, then a lane per (env, probe) forms the point and samples the field under it; without probes both
//               phases and their barrier are skipped.  Last, the lanes run across the group's [ne * P] grid points, which are one
//               contiguous block of `heights` and of `obs` and two of `points`: lane i rotates offset i % P by the yaw pair of env i / P,
//               gathers its two (nearest) or four (bilinear) 2-byte samples and stores word i, so a wave's stores cover whole 256-byte
//               pieces of the row.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "dw_height_scan.h"
#include "dw_group.h"

namespace {

grp::Err s_err;

constexpr int G = DWH_GROUP, TPB = DWH_GROUP * DWH_LANES, NPR = DWH_MAX_PROBES;
// the largest map side for which terrain_sample's upper clamp, (float)(rows - 1) - 1e-3f, still lies below the last sample line in float32
constexpr int MAX_SIDE = 8192;
static_assert(TPB % 64 == 0 && DWH_LANES == 16 && G * NPR <= TPB, "whole waves, sixteen lanes per env, a lane per (env, probe)");
static_assert((DWH_TABLE_WORDS + G * (dwh::IN_ROOT + dwh::IN_DOF + NPR * (dwh::FP + dwh::PW) + 3)) * 4 <= 64 * 1024, "static LDS");

struct Out {
    float *heights, *points, *obs, *probe_pos, *probe_height, *clearance, *probe_normal;
};

__global__ __launch_bounds__(TPB) void dwh_k_scan(int n, const uint4 *__restrict__ table, const float *__restrict__ root_states,
                                                  const float *__restrict__ dof_state, dwh::Map M, int rule, Out out) {
    __shared__ uint4 s_tab4[DWH_TABLE_WORDS / 4];
    __shared__ float s_root[G * dwh::IN_ROOT];
    __shared__ float s_dof[G * dwh::IN_DOF];
    __shared__ float s_fp[G * NPR * dwh::FP];
    __shared__ float s_pr[G * NPR * dwh::PW];
    __shared__ float s_yaw[G * 2];
    __shared__ int s_ok[G];
    const int t = threadIdx.x, e0 = blockIdx.x * G;
    const int ne = n - e0 < G ? n - e0 : G;          // envs of this workgroup (the last one may hold fewer)
    grp::load_table<TPB, DWH_TABLE_WORDS>(table, t, s_tab4);
    grp::load_rows<TPB>(root_states, e0, ne, dwh::IN_ROOT, t, s_root);
    grp::load_rows<TPB>(dof_state, e0, ne, dwh::IN_DOF, t, s_dof);
    __syncthreads();
    const dwh::Tab T{dwb::Tab{reinterpret_cast<const uint32_t *>(s_tab4)}};
    const int P = T.np(), B = T.nb(), NW = T.nw();
    const float inv = 1.0f / M.hscale, nan = dwh::nanf32();
    const dw::PhysParams PP = dwh::phys(M, inv);
    // ---- per env: the finite check over its sixteen lanes, the yaw pair ----
    {
        const int el = t / DWH_LANES, l = t - DWH_LANES * el;
        int bad = el < ne && !dwh::env_part(s_root + el * dwh::IN_ROOT, s_dof + el * dwh::IN_DOF, l, DWH_LANES);
#pragma unroll
        for (int m = 1; m < DWH_LANES; m <<= 1) bad |= __shfl_xor(bad, m, DWH_LANES);
        if (l == 0 && el < ne) {
            s_ok[el] = !bad;
            dwh::yaw_pair(s_root + el * dwh::IN_ROOT, s_yaw + 2 * el, s_yaw + 2 * el + 1);
        }
    }
    // ---- the probes: a lane per (env, walk), then a lane per (env, probe) ----
    const bool probes = B > 0 && (out.probe_pos || out.probe_height || out.clearance || out.probe_normal);
    if (probes) {
        if (NW > 0 && t < ne * NW) {
            const int ce = t / NW;
            dwh::walk(T, t - NW * ce, s_root + ce * dwh::IN_ROOT, s_dof + ce * dwh::IN_DOF, s_fp + (ce * NPR + (t - NW * ce)) * dwh::FP);
        }
        __syncthreads();
        if (t < ne * B) {
            const int ce = t / B, k = t - B * ce;
            float r[dwh::PW];
            if (s_ok[ce]) {
                dwh::probe(T, M, PP, k, s_fp + ce * NPR * dwh::FP, s_root + ce * dwh::IN_ROOT, r);
            } else {
#pragma unroll
                for (int i = 0; i < dwh::PW; ++i) r[i] = nan;
            }
#pragma unroll
            for (int i = 0; i < dwh::PW; ++i) s_pr[(ce * B + k) * dwh::PW + i] = r[i];
        }
    }
    __syncthreads();
    if (probes) {          // the group's blocks of the probe outputs: consecutive lanes, consecutive words
        const int nk = ne * B;
        const size_t k0 = (size_t)e0 * B;
        if (out.probe_pos)
            for (int i = t; i < 3 * nk; i += TPB) out.probe_pos[3 * k0 + i] = s_pr[(i / 3) * dwh::PW + dwh::R_POS + i % 3];
        if (out.probe_normal)
            for (int i = t; i < 3 * nk; i += TPB) out.probe_normal[3 * k0 + i] = s_pr[(i / 3) * dwh::PW + dwh::R_N + i % 3];
        if (out.probe_height)
            for (int i = t; i < nk; i += TPB) out.probe_height[k0 + i] = s_pr[i * dwh::PW + dwh::R_H];
        if (out.clearance)
            for (int i = t; i < nk; i += TPB) out.clearance[k0 + i] = s_pr[i * dwh::PW + dwh::R_CLR];
    }
    // ---- the grid: lanes across the group's points ----
    if (out.heights || out.points || out.obs) {
        const int total = ne * P;
        const size_t g0 = (size_t)e0 * P;
        const bool need_h = out.heights || out.obs;
        for (int i = t; i < total; i += TPB) {
            const int e = i / P, p = i - e * P;
            const float *root = s_root + e * dwh::IN_ROOT;
            float xw = nan, yw = nan, h = nan, o = nan;
            if (s_ok[e]) {
                dwh::grid_point(s_yaw[2 * e], s_yaw[2 * e + 1], T.ox(p), T.oy(p), root, &xw, &yw);
                if (need_h) {
                    h = dwh::grid_height(M, PP, rule, xw, yw);
                    o = dwh::obs_word(T, root[2], h);
                }
            }
            if (out.heights) out.heights[g0 + i] = h;
            if (out.obs) out.obs[g0 + i] = o;
            if (out.points) {
                out.points[2 * (g0 + i)] = xw;
                out.points[2 * (g0 + i) + 1] = yw;
            }
        }
    }
}

bool finite_pos(float x) { return x > 0.0f && x <= 3.4028234664e38f; }

}  // namespace

extern "C" {

int dwh_abi_version(void) { return DWH_ABI_VERSION; }
const char *dwh_last_error(void) { return s_err.s; }

int dwh_pack_table(const void *model, const float *grid_xy, int32_t np, const DwhProbe *probes, int32_t nb, const DwhParams *params,
                   uint32_t *table_host) {
    if (params && (params->rows > MAX_SIDE || params->cols > MAX_SIDE)) return s_err.fail("dwh_pack_table: a map side must not exceed 8192 samples");
    return dwh::pack(static_cast<const DwbModel *>(model), grid_xy, np, probes, nb, params, table_host, s_err.s, sizeof(s_err.s));
}

int dwh_scan(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const int16_t *height_samples,
             int32_t rows, int32_t cols, float hscale, float vscale, float border, int32_t rule, int32_t gpu_div, float *heights,
             float *points, float *obs, float *probe_pos, float *probe_height, float *clearance, float *probe_normal, void *stream) {
    if (num_envs < 1 || num_envs > 0x7fffffff - G) return s_err.fail("dwh_scan: num_envs must be in [1, 2^31 - 16)");
    if (!table || !root_states || !dof_state) return s_err.fail("dwh_scan: a buffer is missing");
    if (!heights && !points && !obs && !probe_pos && !probe_height && !clearance && !probe_normal) return s_err.fail("dwh_scan: at least one output must be given");
    if ((reinterpret_cast<uintptr_t>(table) & 15u) != 0u) return s_err.fail("dwh_scan: the table must be 16-byte aligned");
    if (rule != DWH_RULE_NEAREST && rule != DWH_RULE_BILINEAR) return s_err.fail("dwh_scan: rule must be DWH_RULE_NEAREST or DWH_RULE_BILINEAR");
    dwh::Map M = {height_samples, 0, 0, 1.0f, 1.0f, 0.0f, (int)(gpu_div != 0)};
    if (height_samples != nullptr) {
        if (rows < 2 || cols < 2) return s_err.fail("dwh_scan: the map must hold at least 2 x 2 samples");
        if (rows > MAX_SIDE || cols > MAX_SIDE) return s_err.fail("dwh_scan: a map side must not exceed 8192 samples");
        if (!finite_pos(hscale) || !finite_pos(vscale)) return s_err.fail("dwh_scan: hscale and vscale must be finite and > 0");
        if (!(border >= -3.4028234664e38f && border <= 3.4028234664e38f)) return s_err.fail("dwh_scan: border must be finite");
        M.rows = rows; M.cols = cols; M.hscale = hscale; M.vscale = vscale; M.border = border;
    }
    const Out out = {heights, points, obs, probe_pos, probe_height, clearance, probe_normal};
    hipLaunchKernelGGL(dwh_k_scan, dim3(dwh::groups(num_envs)), dim3(TPB), 0, (hipStream_t)stream, (int)num_envs,
                       reinterpret_cast<const uint4 *>(table), root_states, dof_state, M, (int)rule, out);
    return s_err.launched("dwh_scan");
}

}  // extern "C"
