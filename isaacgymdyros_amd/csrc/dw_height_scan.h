// dw_height_scan.h -- one env's terrain height scan (include/dyros_height_scan.h), written once for the HIP kernel of dw_height_scan.hip and
// for a g++ build (tests/height_scan_host.cpp), which the CPU tests hold bit for bit against a numpy restatement of the header and within a
// measured tolerance against float64.  The pieces: env_part (a strided share of the finite check), yaw_pair, grid_point, coord / nearest /
// bilinear (a grid point's height by either rule), obs_word, walk (the chain from the base down to a probe's carrier, by dw_bodies.h's link
// arithmetic) and probe (a probe's eight output words).  The bilinear rule and the probes call dw::terrain_sample of dw_physics.h itself, so
// these functions exist where that one does: on the device under hipcc, on the host under g++ (with the tests' shim for dw_wave.h).
// pack() is the host's table builder.
#ifndef DW_HEIGHT_SCAN_H
#define DW_HEIGHT_SCAN_H

#include "../../include/dyros_height_scan.h"
#include "dw_bodies.h"
#include "dw_physics.h"

#define DWH_HD DW_HD

namespace dwh {

static_assert(DWH_T_NP == DWB_TABLE_WORDS, "the scan's words follow the chain's");
static_assert(DWH_T_WALK + 2 * DWH_MAX_PROBES == DWH_T_PROBE && DWH_T_PROBE + DWH_PROBE_WORDS * DWH_MAX_PROBES == DWH_T_GRID, "the table's sections");
static_assert(DWH_T_GRID + 2 * DWH_MAX_POINTS == DWH_TABLE_WORDS && DWH_TABLE_WORDS % 4 == 0, "the table's sections");

constexpr int G = DWH_GROUP, IN_ROOT = 13, IN_DOF = 2 * DWB_NUM_DOF, FP = 12, PW = 8;
constexpr int NCHECK = IN_ROOT + DWB_NUM_DOF;          // words of the finite check: the root row and the joint angles
// words of a probe's result
constexpr int R_POS = 0, R_H = 3, R_CLR = 4, R_N = 5;

DWB_HD int groups(int n) { return (n + G - 1) / G; }

struct Tab {
    dwb::Tab c;
    DWB_HD int np() const { const int v = c.i(DWH_T_NP); return v < 1 ? 1 : (v > DWH_MAX_POINTS ? DWH_MAX_POINTS : v); }
    DWB_HD int nb() const { return c.clampi(c.i(DWH_T_NB), DWH_MAX_PROBES); }
    DWB_HD int nw() const { return c.clampi(c.i(DWH_T_NW), DWH_MAX_PROBES); }
    DWB_HD float ox(int p) const { return c.f(DWH_T_GRID + 2 * p); }
    DWB_HD float oy(int p) const { return c.f(DWH_T_GRID + 2 * p + 1); }
    DWB_HD int probe(int k) const { return DWH_T_PROBE + k * DWH_PROBE_WORDS; }
};

// the map as dwh_scan's arguments give it; hs == nullptr: the ground plane
struct Map {
    const int16_t *hs;
    int rows, cols;
    float hscale, vscale, border;
    int gpu_div;
};

DWH_HD float nanf32() {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(0x7fc00000u);
#else
    const uint32_t b = 0x7fc00000u;
    float x;
    memcpy(&x, &b, 4);
    return x;
#endif
}

DWH_HD bool finite32(float x) { return fabsf(x) <= 3.4028234664e38f; }          // (false for NaN)

// whether words k0, k0 + step, ... of the env's checked words (the 13 of the root row, then the 33 joint angles) are all finite
DWH_HD bool env_part(const float *root, const float *dof, int k0, int step) {
    bool ok = true;
    for (int k = k0; k < NCHECK; k += step) ok = ok && finite32(k < IN_ROOT ? root[k] : dof[2 * (k - IN_ROOT)]);
    return ok;
}

// step 1 of the header: the yaw quaternion's z and w
DWH_HD void yaw_pair(const float *root, float *z, float *w) {
    const float qz = root[5], qw = root[6];
    float n = sqrtf(qz * qz + qw * qw);
    n = n > 1e-9f ? n : 1e-9f;
    *z = qz / n;
    *w = qw / n;
}

// steps 2 and 3: the world point of offset (ox, oy)
DWH_HD void grid_point(float z, float w, float ox, float oy, const float *root, float *xw, float *yw) {
    const float tx = -(z * oy) * 2.0f, ty = (z * ox) * 2.0f;
    const float X = (ox + w * tx) - z * ty, Y = (oy + w * ty) + z * tx;
    *xw = X + root[0];
    *yw = Y + root[1];
}

// step 4: inv = 1.0f / hscale, formed once
DWH_HD float coord(const Map &M, float inv, float x) { return M.gpu_div ? (x + M.border) * inv : (x + M.border) / M.hscale; }

// step 5: clamped in float, then truncated (u > 0 first: a NaN fails it and lands on 0)
DWH_HD int cell(float u, int n) {
    const float hi = (float)(n - 2);
    u = u > 0.0f ? (u > hi ? hi : u) : 0.0f;
    return (int)u;
}

// steps 4 to 6: the reference's get_heights at a world point
DWH_HD float nearest(const Map &M, float inv, float xw, float yw) {
    const int i = cell(coord(M, inv, xw), M.rows), j = cell(coord(M, inv, yw), M.cols);
    const int16_t *p = M.hs + (size_t)i * M.cols + j;
    const int16_t a = p[0], b = p[M.cols + 1];
    return (float)(a < b ? a : b) * M.vscale;
}

// what terrain_sample reads of the physics' parameters, formed as dw_params.h forms them
DWH_HD dw::PhysParams phys(const Map &M, float inv) {
    dw::PhysParams P = {};
    P.hs = M.hs;
    P.t_rows = M.rows; P.t_cols = M.cols;
    P.t_inv_h = inv; P.t_vs = M.vscale; P.t_border = M.border;
    return P;
}

// a grid point's height by `rule`
DWH_HD float grid_height(const Map &M, const dw::PhysParams &P, int rule, float xw, float yw) {
    if (M.hs == nullptr) return 0.0f;
    if (rule == DWH_RULE_BILINEAR) {
        float h, fr[9];
        dw::terrain_sample(P, xw, yw, &h, fr);
        return h;
    }
    return nearest(M, P.t_inv_h, xw, yw);
}

DWH_HD float obs_word(const Tab &T, float root_z, float h) {
    const float off = T.c.f(DWH_T_OBS), c = T.c.f(DWH_T_OBS + 1), s = T.c.f(DWH_T_OBS + 2);
    float d = (root_z - off) - h;
    d = d < -c ? -c : (d > c ? c : d);
    return d * s;
}

// walk wk of the table: fp[0:3] = the carrier's offset from the base, fp[3:12] = its rotation (depth 0: the base itself)
DWH_HD void walk(const Tab &T, int wk, const float *root, const float *dof, float *fp) {
    const int l = T.c.clampi(T.c.i(DWH_T_WALK + 2 * wk), DWB_MAX_LEAVES - 1), depth = T.c.clampi(T.c.i(DWH_T_WALK + 2 * wk + 1), DWB_MAX_DEPTH);
    dwb::Body B;
    dwb::base(T.c, root, 0, B);
    for (int k = 0; k < depth; ++k) {
        const int b = T.c.clampi(T.c.path(l, k) & 255, dwb::NM - 1);
        if (b < 1) break;
        dwb::child(T.c, b, dof, B);
    }
    for (int i = 0; i < 3; ++i) fp[i] = B.off[i];
    for (int i = 0; i < 9; ++i) fp[3 + i] = B.R[i];
}

// probe k: out [PW] = pos[3], height, clearance, normal[3]; fps = the env's walks [DWH_MAX_PROBES][FP]
DWH_HD void probe(const Tab &T, const Map &M, const dw::PhysParams &P, int k, const float *fps, const float *root, float *out) {
    const int pk = T.probe(k);
    const float *fp = fps + T.c.clampi(T.c.i(pk + 1), DWH_MAX_PROBES - 1) * FP;
    const float c[3] = {T.c.f(pk + 2), T.c.f(pk + 3), T.c.f(pk + 4)};
    float r[3];
    dwb::m3v(fp + 3, c, r);
    for (int i = 0; i < 3; ++i) out[R_POS + i] = root[i] + (fp[i] + r[i]);
    float h = 0.0f, fr[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if (M.hs != nullptr) dw::terrain_sample(P, out[R_POS], out[R_POS + 1], &h, fr);
    out[R_H] = h;
    out[R_CLR] = M.hs != nullptr ? out[R_POS + 2] - h : out[R_POS + 2];
    out[R_N] = fr[6]; out[R_N + 1] = fr[7]; out[R_N + 2] = fr[8];
}

// ---- host: the table (dwh_pack_table) ----
inline int pack(const DwbModel *M, const float *grid, int np, const DwhProbe *probes, int nb, const DwhParams *prm, uint32_t *t, char *err, size_t errn) {
    auto fail = [&](const char *msg, int idx) { snprintf(err, errn, "dwh_pack_table: %s (index %d)", msg, idx); return -1; };
    auto putf = [&](int k, float f) { memcpy(t + k, &f, 4); };
    auto fin = [](float x) { return fabsf(x) <= 3.4028234664e38f; };
    if (!M || !grid || !prm || !t || (nb > 0 && !probes)) return fail("a pointer is missing", 0);
    if (np < 1 || np > DWH_MAX_POINTS) return fail("the number of grid points must be in 1..DWH_MAX_POINTS", np);
    if (nb < 0 || nb > DWH_MAX_PROBES) return fail("the number of probes must be in 0..DWH_MAX_PROBES", nb);
    for (int p = 0; p < 2 * np; ++p)
        if (!fin(grid[p])) return fail("a grid offset is not finite", p / 2);
    if (prm->rows != 0 || prm->cols != 0) {
        if (prm->rows < 2 || prm->cols < 2) return fail("the map must hold at least 2 x 2 samples", prm->rows < 2 ? prm->rows : prm->cols);
        if ((long long)prm->rows * prm->cols > 0x7fffffffLL) return fail("the map must hold fewer than 2^31 samples", 0);
        if (!fin(prm->hscale) || !(prm->hscale > 0.0f)) return fail("hscale must be finite and > 0", 0);
        if (!fin(prm->vscale) || !(prm->vscale > 0.0f)) return fail("vscale must be finite and > 0", 0);
        if (!fin(prm->border)) return fail("border must be finite", 0);
    }
    if (!fin(prm->obs_offset) || !fin(prm->obs_scale) || !fin(prm->obs_clip) || prm->obs_clip < 0.0f) return fail("the obs parameters must be finite, obs_clip >= 0", 0);
    uint32_t chain[DWB_TABLE_WORDS];
    if (dwb::pack(M, chain, err, errn, "dwh_pack_table") != 0) return -1;
    memset(t, 0, sizeof(uint32_t) * DWH_TABLE_WORDS);
    memcpy(t, chain, sizeof(chain));
    const dwb::Tab C{t};
    t[DWH_T_NP] = (uint32_t)np;
    t[DWH_T_NB] = (uint32_t)nb;
    t[DWH_T_ROWS] = (uint32_t)prm->rows; t[DWH_T_COLS] = (uint32_t)prm->cols;
    putf(DWH_T_HSCALE, prm->hscale); putf(DWH_T_VSCALE, prm->vscale); putf(DWH_T_BORDER, prm->border);
    putf(DWH_T_OBS, prm->obs_offset); putf(DWH_T_OBS + 1, prm->obs_clip); putf(DWH_T_OBS + 2, prm->obs_scale);
    for (int p = 0; p < 2 * np; ++p) putf(DWH_T_GRID + p, grid[p]);
    int nw = 0, carrier[DWH_MAX_PROBES];
    for (int k = 0; k < nb; ++k) {
        const int g = probes[k].body;
        if (g < 0 || g >= dwb::NB) return fail("a probe sits on an unknown body", k);
        for (int i = 0; i < 3; ++i)
            if (!fin(probes[k].pos[i])) return fail("a probe's point is not finite", k);
        const int m = C.carrier(g);
        int wk = 0;
        while (wk < nw && carrier[wk] != m) ++wk;
        if (wk == nw) {          // a new walk: the first path that holds the carrier, down to it
            int l = 0, depth = 0;
            for (int p = 0; p < C.nleaf() && m > 0 && depth == 0; ++p)
                for (int q = 0; q < C.pathlen(p) && depth == 0; ++q)
                    if ((C.path(p, q) & 255) == m) { l = p; depth = q + 1; }
            if (m > 0 && depth == 0) return fail("a probe's carrier is on no path of the tree", k);
            carrier[nw] = m;
            t[DWH_T_WALK + 2 * nw] = (uint32_t)l;
            t[DWH_T_WALK + 2 * nw + 1] = (uint32_t)depth;
            ++nw;
        }
        const int pk = DWH_T_PROBE + k * DWH_PROBE_WORDS;
        t[pk] = (uint32_t)g;
        t[pk + 1] = (uint32_t)wk;
        for (int i = 0; i < 3; ++i) putf(pk + 2 + i, probes[k].pos[i]);
    }
    t[DWH_T_NW] = (uint32_t)nw;
    return 0;
}

}  // namespace dwh

#endif
