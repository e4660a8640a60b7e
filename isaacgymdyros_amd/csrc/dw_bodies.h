// dw_bodies.h -- one env's rigid-body states (include/dyros_bodies.h), written once for the HIP kernel of dw_bodies.hip and for a g++ build
// (tests/body_states_host.cpp), which the CPU tests hold against a float64 numpy restatement.  Three pieces: walk_path (one root-to-leaf path
// of the tree; the kernel gives every path a lane), out_word (one word of an output row) and com_part (a strided share of the inertial
// records).  Between them stands the env's store of moving-body states, [DWB_NUM_MOVING][DWB_ROW] floats: offset from the base, quaternion,
// origin velocity, angular velocity.  pack() is the host's table builder.
#ifndef DW_BODIES_H
#define DW_BODIES_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/dyros_bodies.h"

#if defined(__HIPCC__)
#define DWB_HD __host__ __device__ inline
#else
#define DWB_HD inline
#endif

namespace dwb {

constexpr int NB = DWB_NUM_BODIES, NM = DWB_NUM_MOVING, NI = DWB_NUM_INERT, ROW = DWB_ROW, MVW = NM * ROW;
constexpr int IN_ROOT = 13, IN_DOF = 2 * DWB_NUM_DOF;
// words of a moving body's stored state
constexpr int S_OFF = 0, S_Q = 3, S_V = 7, S_W = 10;

DWB_HD int groups(int n) { return (n + DWB_GROUP - 1) / DWB_GROUP; }

// the table as the kernel reads it (global memory, LDS or host memory)
struct Tab {
    const uint32_t *w;
    DWB_HD int i(int k) const { return (int)w[k]; }
    DWB_HD float f(int k) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return __uint_as_float(w[k]);
#else
        float x;
        memcpy(&x, w + k, 4);
        return x;
#endif
    }
    DWB_HD int clampi(int v, int hi) const { return v < 0 ? 0 : (v > hi ? hi : v); }          // (a damaged table must not index past a store)
    DWB_HD int nleaf() const { return clampi(i(DWB_T_NLEAF), DWB_MAX_LEAVES); }
    DWB_HD int pathlen(int l) const { return clampi(i(DWB_T_PATHLEN + l), DWB_MAX_DEPTH); }
    DWB_HD int path(int l, int k) const { return i(DWB_T_PATH + l * DWB_MAX_DEPTH + k); }
    DWB_HD int mv(int b) const { return DWB_T_MV + b * DWB_MV_WORDS; }
    DWB_HD int carrier(int g) const { return clampi(i(DWB_T_CARRIER + g), NM - 1); }
    DWB_HD int record(int g) const { const int r = i(DWB_T_RECORD + g); return r < 0 ? -1 : (r > NI - 1 ? NI - 1 : r); }
    DWB_HD int inert(int k) const { return DWB_T_INERT + k * DWB_INERT_WORDS; }
};

DWB_HD void quat_mul(const float *a, const float *b, float *o) {          // xyzw
    const float x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    const float y = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    const float z = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    const float w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}

DWB_HD void quat_to_mat(const float *q, float *R) {          // (the physics' quat_to_mat)
    const float X = q[0], Y = q[1], Z = q[2], W = q[3];
    R[0] = 1 - 2 * (Y * Y + Z * Z); R[1] = 2 * (X * Y - W * Z); R[2] = 2 * (X * Z + W * Y);
    R[3] = 2 * (X * Y + W * Z); R[4] = 1 - 2 * (X * X + Z * Z); R[5] = 2 * (Y * Z - W * X);
    R[6] = 2 * (X * Z - W * Y); R[7] = 2 * (Y * Z + W * X); R[8] = 1 - 2 * (X * X + Y * Y);
}

DWB_HD void m3v(const float *R, const float *v, float *o) {
    for (int i = 0; i < 3; ++i) o[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
}

DWB_HD void cross(const float *a, const float *b, float *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// a moving body on the way down a path
struct Body {
    float off[3], q[4], R[9], v[3], w[3];
};

DWB_HD void put(const Body &B, float *s) {
    for (int i = 0; i < 3; ++i) { s[S_OFF + i] = B.off[i]; s[S_V + i] = B.v[i]; s[S_W + i] = B.w[i]; }
    for (int i = 0; i < 4; ++i) s[S_Q + i] = B.q[i];
}

// the base from the root row: the quaternion normalised as the physics does, the origin velocity with the COM's share taken out
DWB_HD void base(const Tab &T, const float *root, int vel_at_com, Body &B) {
    const float n = sqrtf(root[3] * root[3] + root[4] * root[4] + root[5] * root[5] + root[6] * root[6]);
    for (int i = 0; i < 4; ++i) B.q[i] = root[3 + i] / n;
    quat_to_mat(B.q, B.R);
    for (int i = 0; i < 3; ++i) { B.off[i] = 0.0f; B.v[i] = root[7 + i]; B.w[i] = root[10 + i]; }
    const int k0 = T.record(0);
    if (vel_at_com && k0 >= 0) {
        const float c[3] = {T.f(T.inert(k0) + 3), T.f(T.inert(k0) + 4), T.f(T.inert(k0) + 5)};
        float rc[3], t[3];
        m3v(B.R, c, rc);
        cross(B.w, rc, t);
        for (int i = 0; i < 3; ++i) B.v[i] -= t[i];
    }
}

// body b from its parent's state (in place): dof = the env's [33][2] rows
DWB_HD void child(const Tab &T, int b, const float *dof, Body &B) {
    const int m = T.mv(b);
    const float pos[3] = {T.f(m + 1), T.f(m + 2), T.f(m + 3)}, q0[4] = {T.f(m + 4), T.f(m + 5), T.f(m + 6), T.f(m + 7)};
    const float ax[3] = {T.f(m + 8), T.f(m + 9), T.f(m + 10)};
    const float ang = dof[2 * (b - 1)], rate = dof[2 * (b - 1) + 1];
    float d[3], t[3];
    m3v(B.R, pos, d);                       // x_b - x_p
    cross(B.w, d, t);
    for (int i = 0; i < 3; ++i) { B.off[i] += d[i]; B.v[i] += t[i]; }
    const float h = 0.5f * ang, sn = sinf(h), cs = cosf(h);
    const float qj[4] = {ax[0] * sn, ax[1] * sn, ax[2] * sn, cs};
    float ql[4];
    quat_mul(q0, qj, ql);
    quat_mul(B.q, ql, B.q);
    quat_to_mat(B.q, B.R);
    m3v(B.R, ax, t);
    for (int i = 0; i < 3; ++i) B.w[i] += t[i] * rate;
}

// path l of the tree: the states of the bodies this path owns go to mvs [NM][ROW]; path 0 also stores the base
DWB_HD void walk_path(const Tab &T, int l, const float *root, const float *dof, int vel_at_com, float *mvs) {
    Body B;
    base(T, root, vel_at_com, B);
    if (l == 0) put(B, mvs);
    const int n = T.pathlen(l);
    for (int k = 0; k < n; ++k) {
        const int e = T.path(l, k), b = T.clampi(e & 255, NM - 1);
        if (b < 1) break;
        child(T, b, dof, B);
        if (e & DWB_PATH_OWNER) put(B, mvs + b * ROW);
    }
}

// w x R(q) c of a stored state
DWB_HD void com_arm(const float *s, const float *c, float *rc, float *wxrc) {
    float R[9];
    quat_to_mat(s + S_Q, R);
    m3v(R, c, rc);
    cross(s + S_W, rc, wxrc);
}

// an output row resolved once: Gym body | carrier << 8 | (inertial record + 1) << 16
DWB_HD int row_of(const Tab &T, int g) { return g | (T.carrier(g) << 8) | ((T.record(g) + 1) << 16); }

// word w of the row of a resolved Gym body
DWB_HD float out_word(const Tab &T, const float *mvs, const float *root, int row, int w, int vel_at_com) {
    if ((row & 255) == 0) return root[w];
    const float *s = mvs + ((row >> 8) & 255) * ROW;
    if (w < 3) return root[w] + s[S_OFF + w];
    if (w < 7 || w >= 10) return s[w];          // (the stored state keeps the row's order)
    float v = s[w];
    const int k = (row >> 16) - 1;
    if (vel_at_com && k >= 0) {
        const float c[3] = {T.f(T.inert(k) + 3), T.f(T.inert(k) + 4), T.f(T.inert(k) + 5)};
        float rc[3], t[3];
        com_arm(s, c, rc, t);
        v += w == 7 ? t[0] : (w == 8 ? t[1] : t[2]);          // (no run-time index into a local array: that would be scratch memory)
    }
    return v;
}

// the inertial records k0, k0 + step, ... added to acc[7]: sum w (off + R c) [3], sum w (vo + w x R c) [3], sum w
DWB_HD void com_part(const Tab &T, const float *mvs, const float *mass_scale, int k0, int step, float *acc) {
    for (int k = k0; k < NI; k += step) {
        const int ik = T.inert(k);
        const int g = T.clampi(T.i(ik), NB - 1), m = T.clampi(T.i(ik + 1), NM - 1);
        const float wk = mass_scale ? T.f(ik + 2) * mass_scale[g] : T.f(ik + 2);
        const float c[3] = {T.f(ik + 3), T.f(ik + 4), T.f(ik + 5)};
        const float *s = mvs + m * ROW;
        float rc[3], t[3];
        com_arm(s, c, rc, t);
        for (int i = 0; i < 3; ++i) {
            acc[i] += wk * (s[S_OFF + i] + rc[i]);
            acc[3 + i] += wk * (s[S_V + i] + t[i]);
        }
        acc[6] += wk;
    }
}

// com [7] from the summed acc
DWB_HD void com_finish(const float *acc, const float *root, float *com) {
    for (int i = 0; i < 3; ++i) {
        com[i] = root[i] + acc[i] / acc[6];
        com[3 + i] = acc[3 + i] / acc[6];
    }
    com[6] = acc[6];
}

// ---- host: the table from the model (dwb_pack_table) ----
// who: the entry point the refusals name (the tables of dw_jacobian.h and of what builds on it begin with this one)
inline int pack(const DwbModel *M, uint32_t *t, char *err, size_t errn, const char *who = "dwb_pack_table") {
    auto fail = [&](const char *msg, int idx) { snprintf(err, errn, "%s: %s (index %d)", who, msg, idx); return -1; };
    auto putf = [&](int k, double v) { const float f = (float)v; memcpy(t + k, &f, 4); };
    if (!M || !t) return fail("a pointer is missing", 0);
    memset(t, 0, sizeof(uint32_t) * DWB_TABLE_WORDS);
    if (M->mv_parent[0] != -1) return fail("moving body 0 must be the base, parent -1", 0);
    bool leaf[NM];
    int depth[NM];
    depth[0] = 0;
    for (int b = 0; b < NM; ++b) leaf[b] = true;
    for (int b = 1; b < NM; ++b) {
        const int p = M->mv_parent[b];
        if (p < 0 || p >= NM) return fail("mv_parent out of range", b);
        if (p >= b) return fail("a child precedes its parent", b);
        leaf[p] = false;
        depth[b] = depth[p] + 1;
        if (depth[b] > DWB_MAX_DEPTH) return fail("the tree is deeper than DWB_MAX_DEPTH", b);
    }
    // paths, in the order of their leaves; the first path through a body owns it
    bool owned[NM] = {false};
    int nleaf = 0;
    for (int b = 1; b < NM; ++b) {
        if (!leaf[b]) continue;
        if (nleaf == DWB_MAX_LEAVES) return fail("the tree has more than DWB_MAX_LEAVES leaves", b);
        int n = depth[b];
        t[DWB_T_PATHLEN + nleaf] = (uint32_t)n;
        for (int c = b; c > 0; c = M->mv_parent[c]) {
            --n;
            t[DWB_T_PATH + nleaf * DWB_MAX_DEPTH + n] = (uint32_t)(c | (owned[c] ? 0 : DWB_PATH_OWNER));
            owned[c] = true;
        }
        ++nleaf;
    }
    t[DWB_T_NLEAF] = (uint32_t)nleaf;
    for (int b = 0; b < NM; ++b) {
        const int m = DWB_T_MV + b * DWB_MV_WORDS;
        t[m] = (uint32_t)M->mv_parent[b];
        for (int i = 0; i < 3; ++i) { putf(m + 1 + i, M->mv_pos[b][i]); putf(m + 8 + i, M->mv_axis[b][i]); }
        // quat(mv_rot0): the largest of w, x, y, z first (Shepperd)
        const float *R = M->mv_rot0[b];
        const double r[9] = {R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8]};
        const double tr = r[0] + r[4] + r[8];
        double q[4];          // xyzw
        if (tr >= r[0] && tr >= r[4] && tr >= r[8]) {
            q[3] = 1 + tr; q[0] = r[7] - r[5]; q[1] = r[2] - r[6]; q[2] = r[3] - r[1];
        } else if (r[0] >= r[4] && r[0] >= r[8]) {
            q[0] = 1 + r[0] - r[4] - r[8]; q[1] = r[1] + r[3]; q[2] = r[2] + r[6]; q[3] = r[7] - r[5];
        } else if (r[4] >= r[8]) {
            q[1] = 1 - r[0] + r[4] - r[8]; q[0] = r[1] + r[3]; q[2] = r[5] + r[7]; q[3] = r[2] - r[6];
        } else {
            q[2] = 1 - r[0] - r[4] + r[8]; q[0] = r[2] + r[6]; q[1] = r[5] + r[7]; q[3] = r[3] - r[1];
        }
        const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        if (!(n > 0.0)) return fail("mv_rot0 is not a rotation", b);
        // the sign: the first of w, x, y, z that is not (nearly) zero is positive (a half turn has w = 0)
        const double lead = fabs(q[3]) > 1e-6 * n ? q[3] : (fabs(q[0]) > 1e-6 * n ? q[0] : (fabs(q[1]) > 1e-6 * n ? q[1] : q[2]));
        const double sg = lead < 0 ? -1.0 : 1.0;
        for (int i = 0; i < 4; ++i) putf(m + 4 + i, sg * q[i] / n);
    }
    for (int g = 0; g < NB; ++g) {
        const int m = M->body_moving[g];
        if (m < 0 || m >= NM) return fail("body_moving out of range: every Gym body needs one carrier", g);
        t[DWB_T_CARRIER + g] = (uint32_t)m;
        t[DWB_T_RECORD + g] = (uint32_t)-1;
    }
    for (int k = 0; k < NI; ++k) {
        const int g = M->inert_gym[k], m = M->inert_mv[k];
        if (g < 0 || g >= NB) return fail("inert_gym out of range", k);
        if (m < 0 || m >= NM) return fail("inert_mv out of range", k);
        if (m != M->body_moving[g]) return fail("an inertial record's moving body is not its Gym body's carrier", k);
        if ((int)t[DWB_T_RECORD + g] != -1) return fail("a Gym body has two inertial records", k);
        t[DWB_T_RECORD + g] = (uint32_t)k;
        const int ik = DWB_T_INERT + k * DWB_INERT_WORDS;
        t[ik] = (uint32_t)g;
        t[ik + 1] = (uint32_t)m;
        putf(ik + 2, M->inert_mass[k]);
        for (int i = 0; i < 3; ++i) putf(ik + 3 + i, M->inert_com[k][i]);
    }
    return 0;
}

}  // namespace dwb

#endif
