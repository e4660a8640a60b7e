// dw_jacobian.h -- one env's Jacobians and joint-space inertia (include/dyros_jacobians.h), written once for the HIP kernels of
// dw_jacobian.hip and for a g++ build (tests/jacobians_host.cpp), which the CPU tests hold against a float64 numpy restatement.  The chain is
// dw_bodies.h's (base, child).  An env's store is one float array: KS, per moving body its offset from the base, quaternion and world joint
// axis (body 0's axis slot holds p_ref); then for the Jacobian PC, the inertial records' COM offsets; for the mass matrix REC (a record's
// weight, COM offset and world rotational inertia), ROWF (per row of M, the subtree's inertia about the row's origin applied to the row's unit
// motion: moment, force), COLB (axis and origin of the six base columns) and BASE (the total mass).  Pieces: walk_path, record_com / record_inertia, body_sum, and the words
// jac_word, mm_word.  pack() is the host's table builder.
#ifndef DW_JACOBIAN_H
#define DW_JACOBIAN_H

#include "../../include/dyros_jacobians.h"
#include "dw_bodies.h"

namespace dwj {

using dwb::Tab;
constexpr int NB = DWJ_NUM_BODIES, NM = DWJ_NUM_MOVING, NI = DWJ_NUM_INERT, NV = DWJ_NV, JR = DWJ_JAC_ROWS;
constexpr int JROW = JR * NV, MMW = NV * NV, CJW = 3 * NV;          // words of a body's Jacobian, of an env's M and COM Jacobian
static_assert(NB == DWB_NUM_BODIES && NM == DWB_NUM_MOVING && NI == DWB_NUM_INERT && DWJ_NUM_DOF == DWB_NUM_DOF && NV == 6 + DWJ_NUM_DOF, "one robot");
static_assert(DWJ_T_ANC == DWB_TABLE_WORDS && DWJ_T_SUB == DWJ_T_ANC + 2 * NM && DWJ_T_I == DWJ_T_SUB + 2 * NM && DWJ_TABLE_WORDS == DWJ_T_I + 6 * NI, "the table's sections");
static_assert(NM <= 64 && NI <= 64, "two mask words");
// a moving body's words in KS
constexpr int KW = 10, K_OFF = 0, K_Q = 3, K_A = 7;
// an env's store; the strides are odd so that the envs of a workgroup start in different LDS banks
constexpr int E_KS = 0, E_PC = NM * KW, JAC_ENV = E_PC + 3 * NI + 1;
constexpr int RW = 10, FW = 6, E_REC = NM * KW, E_ROWF = E_REC + NI * RW, E_COLB = E_ROWF + NV * FW, E_BASE = E_COLB + 36, MM_ENV = E_BASE + 1;
static_assert(JAC_ENV % 2 == 1 && MM_ENV % 2 == 1, "odd strides");

DWB_HD int groups(int n) { return (n + DWJ_GROUP - 1) / DWJ_GROUP; }
DWB_HD bool bit(const Tab &T, int at, int row, int b) { return (T.w[at + 2 * row + (b >> 5)] >> (b & 31)) & 1u; }

// path l of the tree: offset, quaternion and world axis of the bodies this path owns go to ks [NM][KW]; path 0 also stores the base, p_ref in
// its axis slot
DWB_HD void walk_path(const Tab &T, int l, const float *root, const float *dof, int vel_at_com, float *ks) {
    dwb::Body B;
    dwb::base(T, root, 0, B);
    if (l == 0) {
        float pref[3] = {0.0f, 0.0f, 0.0f};
        const int k0 = T.record(0);
        if (vel_at_com && k0 >= 0) {
            const float c[3] = {T.f(T.inert(k0) + 3), T.f(T.inert(k0) + 4), T.f(T.inert(k0) + 5)};
            dwb::m3v(B.R, c, pref);
        }
        for (int i = 0; i < 3; ++i) { ks[K_OFF + i] = 0.0f; ks[K_A + i] = pref[i]; }
        for (int i = 0; i < 4; ++i) ks[K_Q + i] = B.q[i];
    }
    const int n = T.pathlen(l);
    for (int k = 0; k < n; ++k) {
        const int e = T.path(l, k), b = T.clampi(e & 255, NM - 1);
        if (b < 1) break;
        dwb::child(T, b, dof, B);
        if (e & DWB_PATH_OWNER) {
            const int m = T.mv(b);
            const float ax[3] = {T.f(m + 8), T.f(m + 9), T.f(m + 10)};
            float a[3];
            dwb::m3v(B.R, ax, a);
            float *s = ks + b * KW;
            for (int i = 0; i < 3; ++i) { s[K_OFF + i] = B.off[i]; s[K_A + i] = a[i]; }
            for (int i = 0; i < 4; ++i) s[K_Q + i] = B.q[i];
        }
    }
}

// record k's COM offset from the base, x_m + R_m c_k, to pc[3]; R (of the carrier) is left for the caller
DWB_HD void record_com(const Tab &T, const float *ks, int k, float *R, float *pc) {
    const int ik = T.inert(k), m = T.clampi(T.i(ik + 1), NM - 1);
    const float c[3] = {T.f(ik + 3), T.f(ik + 4), T.f(ik + 5)};
    const float *s = ks + m * KW;
    float rc[3];
    dwb::quat_to_mat(s + K_Q, R);
    dwb::m3v(R, c, rc);
    for (int i = 0; i < 3; ++i) pc[i] = s[K_OFF + i] + rc[i];
}

// record k to rec[RW]: w_k, the COM offset, s_k R I_k R' (xx, yy, zz, xy, xz, yz); mass_scale: the env's [38] or NULL
DWB_HD void record_inertia(const Tab &T, const float *ks, const float *mass_scale, int k, float *rec) {
    float R[9], pc[3];
    record_com(T, ks, k, R, pc);
    const int ik = T.inert(k), g = T.clampi(T.i(ik), NB - 1), ii = DWJ_T_I + 6 * k;
    const float sc = mass_scale ? mass_scale[g] : 1.0f;
    const float xx = T.f(ii), yy = T.f(ii + 1), zz = T.f(ii + 2), xy = T.f(ii + 3), xz = T.f(ii + 4), yz = T.f(ii + 5);
    // A = R I, then A R'
    float A[9];
    for (int r = 0; r < 3; ++r) {
        A[3 * r] = R[3 * r] * xx + R[3 * r + 1] * xy + R[3 * r + 2] * xz;
        A[3 * r + 1] = R[3 * r] * xy + R[3 * r + 1] * yy + R[3 * r + 2] * yz;
        A[3 * r + 2] = R[3 * r] * xz + R[3 * r + 1] * yz + R[3 * r + 2] * zz;
    }
    auto ar = [&](int r, int c) { return A[3 * r] * R[3 * c] + A[3 * r + 1] * R[3 * c + 1] + A[3 * r + 2] * R[3 * c + 2]; };
    rec[0] = T.f(ik + 2) * sc;
    rec[1] = pc[0]; rec[2] = pc[1]; rec[3] = pc[2];
    rec[4] = sc * ar(0, 0); rec[5] = sc * ar(1, 1); rec[6] = sc * ar(2, 2);
    rec[7] = sc * ar(0, 1); rec[8] = sc * ar(0, 2); rec[9] = sc * ar(1, 2);
}

// moving body i: mass, first and second moment about x_i (the base: about p_ref) of the records of its subtree, in the records' order,
// applied to the row's unit motion: ROWF row 5 + i = (I a_i, a_i x h) for a joint; rows 0..5 for the base's three translations and three
// rotations, whose columns' axes and origins go to COLB and the total mass to BASE
DWB_HD void body_sum(const Tab &T, float *E, int i) {
    const float *ks = E + E_KS + i * KW, *x = i == 0 ? ks + K_A : ks + K_OFF;
    const float x0 = x[0], x1 = x[1], x2 = x[2];
    float mc = 0.0f, h0 = 0.0f, h1 = 0.0f, h2 = 0.0f, ixx = 0.0f, iyy = 0.0f, izz = 0.0f, ixy = 0.0f, ixz = 0.0f, iyz = 0.0f;
    for (uint64_t left = (uint64_t)T.w[DWJ_T_SUB + 2 * i] | ((uint64_t)T.w[DWJ_T_SUB + 2 * i + 1] << 32); left != 0; left &= left - 1) {
        const int k = T.clampi(__builtin_ctzll(left), NI - 1);
        const float *rec = E + E_REC + k * RW;
        const float w = rec[0], r0 = rec[1] - x0, r1 = rec[2] - x1, r2 = rec[3] - x2;
        mc += w;
        h0 += w * r0; h1 += w * r1; h2 += w * r2;
        ixx += rec[4] + w * (r1 * r1 + r2 * r2);
        iyy += rec[5] + w * (r0 * r0 + r2 * r2);
        izz += rec[6] + w * (r0 * r0 + r1 * r1);
        ixy += rec[7] - w * (r0 * r1);
        ixz += rec[8] - w * (r0 * r2);
        iyz += rec[9] - w * (r1 * r2);
    }
    if (i == 0) {
        // a translation e_c: moment h x e_c, force M e_c; a rotation e_c about p_ref: moment I e_c, force e_c x h
        const float rows[6][FW] = {{0.0f, h2, -h1, mc, 0.0f, 0.0f}, {-h2, 0.0f, h0, 0.0f, mc, 0.0f}, {h1, -h0, 0.0f, 0.0f, 0.0f, mc},
                                   {ixx, ixy, ixz, 0.0f, -h2, h1}, {ixy, iyy, iyz, h2, 0.0f, -h0}, {ixz, iyz, izz, -h1, h0, 0.0f}};
        for (int r = 0; r < 6; ++r) {
            for (int c = 0; c < FW; ++c) E[E_ROWF + r * FW + c] = rows[r][c];
            for (int c = 0; c < 3; ++c) {
                E[E_COLB + 6 * r + c] = (r == c || r == c + 3) ? 1.0f : 0.0f;
                E[E_COLB + 6 * r + 3 + c] = r < 3 ? 0.0f : x[c];
            }
        }
        E[E_BASE] = mc;
    } else {
        const float a0 = ks[K_A], a1 = ks[K_A + 1], a2 = ks[K_A + 2];
        float *f = E + E_ROWF + (5 + i) * FW;
        f[0] = ixx * a0 + ixy * a1 + ixz * a2;
        f[1] = ixy * a0 + iyy * a1 + iyz * a2;
        f[2] = ixz * a0 + iyz * a1 + izz * a2;
        f[3] = a1 * h2 - a2 * h1;
        f[4] = a2 * h0 - a0 * h2;
        f[5] = a0 * h1 - a1 * h0;
    }
}

// 0, 1, 2 -> 1, 2, 0 and 2, 0, 1 (no run-time index into a local array: that would be scratch memory)
DWB_HD int nxt(int i) { return i == 2 ? 0 : i + 1; }
DWB_HD int prv(int i) { return i == 0 ? 2 : i - 1; }
// component i of a x (p - o), a, p, o in the env's store
DWB_HD float cross_arm(const float *a, const float *p, const float *o, int i) {
    const int i1 = nxt(i), i2 = prv(i);
    return a[i1] * (p[i2] - o[i2]) - a[i2] * (p[i1] - o[i1]);
}

// an output row of the Jacobian resolved once: carrier | word of its point in the env's store << 8 | base << 24
DWB_HD int jac_row_of(const Tab &T, int g, int vel_at_com) {
    const int m = T.carrier(g), k = T.record(g);
    const int at = vel_at_com && k >= 0 ? E_PC + 3 * k : E_KS + m * KW + K_OFF;
    return m | (at << 8) | (g == 0 ? 1 << 24 : 0);
}

// word (i, c) of the [6][39] Jacobian of a resolved row; E = the env's store after walk_path and (vel_at_com) record_com
DWB_HD float jac_word(const Tab &T, const float *E, int row, int i, int c) {
    if (row >> 24) return i == c ? 1.0f : 0.0f;
    const float *p = E + ((row >> 8) & 0xffff);
    if (c < 6) {
        if (i >= 3 || c < 3) return i == c ? 1.0f : 0.0f;
        const int j = c - 3;
        if (i == j) return 0.0f;
        // -[d]x e_j = e_j x d, d = p - p_ref: component i is +d_k or -d_k, k the third axis
        const float *pref = E + E_KS + K_A;
        const int k = 3 - i - j;
        const float d = p[k] - pref[k];
        return nxt(i) == j ? d : -d;
    }
    const int b = c - 5, m = row & 255;
    if (!bit(T, DWJ_T_ANC, m, b)) return 0.0f;
    const float *s = E + E_KS + b * KW;
    return i >= 3 ? s[K_A + i - 3] : cross_arm(s + K_A, p, s + K_OFF, i);
}

// entry (hi, lo), hi >= lo, of the [39][39] mass matrix; E = the env's store after body_sum; arm: the env's [33] armatures or NULL.  One
// form for every entry, so that a wave whose lanes hold entries of every block runs one path: column lo's unit motion at row hi's origin
// (a translation e_c; or a rotation about an axis through an origin: a joint's, or e_c through p_ref) dotted with the row's (moment, force)
DWB_HD float mm_entry(const Tab &T, const float *E, const float *arm, int hi, int lo) {
    const bool cb = lo < 6, pris = lo < 3;
    const int xo = hi < 6 ? E_KS + K_A : E_KS + (hi - 5) * KW + K_OFF;
    const int ao = cb ? E_COLB + 6 * lo : E_KS + (lo - 5) * KW + K_A, oo = cb ? E_COLB + 6 * lo + 3 : E_KS + (lo - 5) * KW + K_OFF;
    const bool valid = cb || bit(T, DWJ_T_ANC, cb ? 0 : hi - 5, cb ? 0 : lo - 5);          // (lo >= 6: hi >= 6 too)
    const float *F = E + E_ROWF + hi * FW;
    const float a0 = E[ao], a1 = E[ao + 1], a2 = E[ao + 2];
    const float r0 = E[xo] - E[oo], r1 = E[xo + 1] - E[oo + 1], r2 = E[xo + 2] - E[oo + 2];
    const float l0 = pris ? a0 : a1 * r2 - a2 * r1, l1 = pris ? a1 : a2 * r0 - a0 * r2, l2 = pris ? a2 : a0 * r1 - a1 * r0;
    float v = pris ? 0.0f : a0 * F[0] + a1 * F[1] + a2 * F[2];
    v += l0 * F[3];
    v += l1 * F[4];
    v += l2 * F[5];
    if (arm && hi == lo && hi >= 6) v += arm[hi - 6];
    return valid ? v : 0.0f;
}

// word (r, c) of the mass matrix: the lower triangle, mirrored
DWB_HD float mm_word(const Tab &T, const float *E, const float *arm, int r, int c) { return r >= c ? mm_entry(T, E, arm, r, c) : mm_entry(T, E, arm, c, r); }
// word (r, c) of the [3][39] COM Jacobian
DWB_HD float cj_word(const Tab &T, const float *E, int r, int c) { return mm_word(T, E, nullptr, r, c) / E[E_BASE]; }

// ---- host: the table from the model (dwj_pack_table) ----
// who: the entry point the refusals name
inline int pack(const DwjModel *M, uint32_t *t, char *err, size_t errn, const char *who = "dwj_pack_table") {
    auto fail = [&](const char *msg, int idx) { snprintf(err, errn, "%s: %s (index %d)", who, msg, idx); return -1; };
    if (!M || !t) return fail("a pointer is missing", 0);
    memset(t, 0, sizeof(uint32_t) * DWJ_TABLE_WORDS);
    DwbModel D;
    memcpy(D.mv_parent, M->mv_parent, sizeof(D.mv_parent));
    memcpy(D.mv_pos, M->mv_pos, sizeof(D.mv_pos));
    memcpy(D.mv_rot0, M->mv_rot0, sizeof(D.mv_rot0));
    memcpy(D.mv_axis, M->mv_axis, sizeof(D.mv_axis));
    memcpy(D.body_moving, M->body_moving, sizeof(D.body_moving));
    memcpy(D.inert_gym, M->inert_gym, sizeof(D.inert_gym));
    memcpy(D.inert_mv, M->inert_mv, sizeof(D.inert_mv));
    memcpy(D.inert_mass, M->inert_mass, sizeof(D.inert_mass));
    memcpy(D.inert_com, M->inert_com, sizeof(D.inert_com));
    if (dwb::pack(&D, t, err, errn, who) != 0) return -1;
    for (int k = 0; k < NI; ++k)
        for (int i = 0; i < 6; ++i) {
            if (!isfinite(M->inert_I[k][i])) return fail("inert_I is not finite", k);
            memcpy(t + DWJ_T_I + 6 * k + i, &M->inert_I[k][i], 4);
        }
    // dwb::pack has checked that parents precede children and that every index is in range
    for (int m = 1; m < NM; ++m)
        for (int b = m; b > 0; b = M->mv_parent[b]) t[DWJ_T_ANC + 2 * m + (b >> 5)] |= 1u << (b & 31);
    for (int k = 0; k < NI; ++k)
        for (int b = M->inert_mv[k]; b >= 0; b = M->mv_parent[b]) t[DWJ_T_SUB + 2 * b + (k >> 5)] |= 1u << (k & 31);
    return 0;
}

}  // namespace dwj

#endif
