// A g++ build of the terrain height scan's per-env arithmetic (isaacgymdyros_amd/csrc/dw_height_scan.h) with host pointers: the functions
// dw_height_scan.hip runs, driven env by env in the kernel's order (the finite check in DWH_LANES strided shares, the yaw pair once, every walk,
// every probe, every grid point).  dw_physics.h is device code under hipcc; here dw_wave.h takes the tests' host shim
// (-Itests/emul -DDW_HOST_SHIM_HEADER='"dw_wave_host.h"', as tests/emul/Makefile does).  tests/test_height_scan.py compiles it and holds it
// bit for bit against the numpy restatement of tests/height_scan_ref.py.
#include <stdint.h>
#include <string.h>

#include "../isaacgymdyros_amd/csrc/dw_height_scan.h"

extern "C" {

int dwhh_pack_table(const DwbModel *m, const float *grid, int np, const DwhProbe *probes, int nb, const DwhParams *prm, uint32_t *table, char *err,
                    int errn) {
    return dwh::pack(m, grid, np, probes, nb, prm, table, err, (size_t)errn);
}

// the outputs of dwh_scan, each or NULL; hs NULL: the plane
int dwhh_scan(int n, const uint32_t *table, const float *root_states, const float *dof_state, const int16_t *hs, int rows, int cols, float hscale,
              float vscale, float border, int rule, int gpu_div, float *heights, float *points, float *obs, float *probe_pos, float *probe_height,
              float *clearance, float *probe_normal) {
    if (n < 1 || !table || !root_states || !dof_state) return -1;
    if (hs && (rows < 2 || cols < 2 || !(hscale > 0.0f) || !(vscale > 0.0f))) return -1;
    const dwh::Tab T{dwb::Tab{table}};
    dwh::Map M = {hs, 0, 0, 1.0f, 1.0f, 0.0f, gpu_div != 0};
    if (hs) { M.rows = rows; M.cols = cols; M.hscale = hscale; M.vscale = vscale; M.border = border; }
    const float inv = 1.0f / M.hscale, nan = dwh::nanf32();
    const dw::PhysParams PP = dwh::phys(M, inv);
    const int P = T.np(), B = T.nb(), NW = T.nw();
    for (int e = 0; e < n; ++e) {
        const float *root = root_states + (size_t)e * dwh::IN_ROOT, *dof = dof_state + (size_t)e * dwh::IN_DOF;
        bool ok = true;
        for (int l = 0; l < DWH_LANES; ++l) ok = dwh::env_part(root, dof, l, DWH_LANES) && ok;
        float z, w;
        dwh::yaw_pair(root, &z, &w);
        if (B > 0 && (probe_pos || probe_height || clearance || probe_normal)) {
            float fps[DWH_MAX_PROBES * dwh::FP];
            memset(fps, 0, sizeof(fps));
            for (int k = 0; k < NW; ++k) dwh::walk(T, k, root, dof, fps + k * dwh::FP);
            for (int k = 0; k < B; ++k) {
                float r[dwh::PW];
                if (ok) dwh::probe(T, M, PP, k, fps, root, r);
                else for (int i = 0; i < dwh::PW; ++i) r[i] = nan;
                const size_t g = (size_t)e * B + k;
                for (int i = 0; i < 3; ++i) {
                    if (probe_pos) probe_pos[3 * g + i] = r[dwh::R_POS + i];
                    if (probe_normal) probe_normal[3 * g + i] = r[dwh::R_N + i];
                }
                if (probe_height) probe_height[g] = r[dwh::R_H];
                if (clearance) clearance[g] = r[dwh::R_CLR];
            }
        }
        if (!heights && !points && !obs) continue;
        for (int p = 0; p < P; ++p) {
            float xw = nan, yw = nan, h = nan, o = nan;
            if (ok) {
                dwh::grid_point(z, w, T.ox(p), T.oy(p), root, &xw, &yw);
                if (heights || obs) {
                    h = dwh::grid_height(M, PP, rule, xw, yw);
                    o = dwh::obs_word(T, root[2], h);
                }
            }
            const size_t g = (size_t)e * P + p;
            if (heights) heights[g] = h;
            if (obs) obs[g] = o;
            if (points) { points[2 * g] = xw; points[2 * g + 1] = yw; }
        }
    }
    return 0;
}

}  // extern "C"
