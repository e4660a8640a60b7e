// dw_dynamics.h -- one env's bias forces, gravity forces, inverse dynamics and momentum (include/dyros_dynamics.h), written once for the HIP
// kernel of dw_dynamics.hip and for a g++ build (tests/dynamics_host.cpp), which the CPU tests hold against a float64 numpy restatement.  A
// recursive Newton-Euler pass on dw_jacobian.h's parts: the chain walk, the records' COM offsets and rotated inertias, the subtree masks.  An
// env's store is one float array: KS (dw_jacobian.h's: per moving body its offset from the base, quaternion and world joint axis; body 0's
// axis slot holds p_ref), KIN (per moving body its angular velocity, origin velocity, and angular and origin acceleration for nu_dot = 0 and
// for the caller's nu_dot), REC (per record its COM offset, weight, and the (force, moment about its COM) pairs of the variants asked for) and
// OUT (the rows of bias, gravity, tau and momentum).  The variants share the kinematics and differ only in velocity and acceleration words, so
// the chain is walked once; gravity (nu = 0, nu_dot = 0) needs none of them: its record force is w (0 - g), its moment 0.
// Pieces: walk_path, record, body_sum.
#ifndef DW_DYNAMICS_H
#define DW_DYNAMICS_H

#include "../../include/dyros_dynamics.h"
#include "dw_jacobian.h"

namespace dwn {

using dwb::Tab;
constexpr int NB = DWN_NUM_BODIES, NM = DWN_NUM_MOVING, NI = DWN_NUM_INERT, NV = DWN_NV, MOM = DWN_MOM;
static_assert(NB == DWJ_NUM_BODIES && NM == DWJ_NUM_MOVING && NI == DWJ_NUM_INERT && DWN_NUM_DOF == DWJ_NUM_DOF && NV == DWJ_NV, "one robot");
static_assert(DWN_TABLE_WORDS == DWJ_TABLE_WORDS, "one table");
// the outputs asked for
constexpr int W_BIAS = 1, W_GRAV = 2, W_TAU = 4, W_MOM = 8;
// a moving body's words in KS (dw_jacobian.h's) and in KIN
constexpr int KW = dwj::KW, K_OFF = dwj::K_OFF, K_Q = dwj::K_Q, K_A = dwj::K_A;
constexpr int QW = 19, Q_W = 0, Q_V = 3, Q_AB = 6, Q_XB = 9, Q_AT = 12, Q_XT = 15;
// a record's words in REC
constexpr int RW = 23, R_PC = 0, R_W = 3, R_FB = 4, R_NB = 7, R_FT = 10, R_NT = 13, R_P = 16, R_L = 19;
// the rows of OUT
constexpr int O_BIAS = 0, O_GRAV = NV, O_TAU = 2 * NV, O_MOM = 3 * NV, OW = 3 * NV + MOM;
// an env's store.  Every stride is odd: lanes that hold consecutive bodies, records or envs then start on different LDS banks (an odd number is
// coprime to the 32 and 64 banks a wave's half is spread over, so 32 consecutive lanes hit 32 different banks at every word of their item)
constexpr int E_KS = 0, E_KIN = E_KS + NM * KW, E_REC = E_KIN + NM * QW, E_OUT = E_REC + NI * RW, ENV = E_OUT + OW;
static_assert(QW % 2 == 1 && RW % 2 == 1 && ENV % 2 == 1, "odd strides");
static_assert(QW >= Q_XT + 3 && RW >= R_L + 3, "the words fit their strides");

DWB_HD int groups(int n) { return (n + DWN_GROUP - 1) / DWN_GROUP; }

// angular and origin acceleration on the way down a path
struct Acc {
    float al[3], xdd[3];
};

// the base: alpha_0 = a[3:6], xdd_0 = a[0:3] - alpha_0 x p_ref - omega_0 x (omega_0 x p_ref)
DWB_HD void base_acc(const float *alin, const float *aang, const float *w, const float *pref, Acc &A) {
    float t[3], u[3], s[3];
    for (int i = 0; i < 3; ++i) A.al[i] = aang[i];
    dwb::cross(A.al, pref, t);
    dwb::cross(w, pref, u);
    dwb::cross(w, u, s);
    for (int i = 0; i < 3; ++i) A.xdd[i] = alin[i] - t[i] - s[i];
}

// to a child's origin, r = x_b - x_p, with the parent's omega and alpha: xdd += alpha x r + omega x (omega x r)
DWB_HD void down(const float *wp, const float *r, Acc &A) {
    float t[3], u[3], s[3];
    dwb::cross(A.al, r, t);
    dwb::cross(wp, r, u);
    dwb::cross(wp, u, s);
    for (int i = 0; i < 3; ++i) A.xdd[i] = A.xdd[i] + t[i] + s[i];
}

// across the child's joint: alpha += a qdd + omega_p x a qd (c = the cross product)
DWB_HD void joint(const float *a, float qdd, const float *c, Acc &A) {
    for (int i = 0; i < 3; ++i) A.al[i] = A.al[i] + a[i] * qdd + c[i];
}

DWB_HD void put(const dwb::Body &B, const float *a, const Acc &Ab, const Acc &At, float *ks, float *kin) {
    for (int i = 0; i < 3; ++i) {
        ks[K_OFF + i] = B.off[i]; ks[K_A + i] = a[i];
        kin[Q_W + i] = B.w[i]; kin[Q_V + i] = B.v[i];
        kin[Q_AB + i] = Ab.al[i]; kin[Q_XB + i] = Ab.xdd[i];
        kin[Q_AT + i] = At.al[i]; kin[Q_XT + i] = At.xdd[i];
    }
    for (int i = 0; i < 4; ++i) ks[K_Q + i] = B.q[i];
}

// path l of the tree: KS and KIN of the bodies this path owns; path 0 also stores the base, p_ref in its axis slot.  acc: the env's nu_dot
// [39] or NULL (then the caller's variant is the nu_dot = 0 one, and nobody reads it)
DWB_HD void walk_path(const Tab &T, int l, const float *root, const float *dof, const float *acc, int vel_at_com, float *E) {
    dwb::Body B;
    dwb::base(T, root, vel_at_com, B);          // (B.v: the base ORIGIN's velocity)
    float pref[3] = {0.0f, 0.0f, 0.0f};
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const int k0 = T.record(0);
    if (vel_at_com && k0 >= 0) {
        const float c[3] = {T.f(T.inert(k0) + 3), T.f(T.inert(k0) + 4), T.f(T.inert(k0) + 5)};
        dwb::m3v(B.R, c, pref);
    }
    Acc Ab, At;
    base_acc(zero, zero, B.w, pref, Ab);
    if (acc) base_acc(acc, acc + 3, B.w, pref, At);
    else At = Ab;
    if (l == 0) put(B, pref, Ab, At, E + E_KS, E + E_KIN);
    const int n = T.pathlen(l);
    for (int k = 0; k < n; ++k) {
        const int e = T.path(l, k), b = T.clampi(e & 255, NM - 1);
        if (b < 1) break;
        const int m = T.mv(b);
        const float pos[3] = {T.f(m + 1), T.f(m + 2), T.f(m + 3)}, ax[3] = {T.f(m + 8), T.f(m + 9), T.f(m + 10)};
        const float wp[3] = {B.w[0], B.w[1], B.w[2]};
        float r[3], a[3], aq[3], c[3];
        dwb::m3v(B.R, pos, r);                   // x_b - x_p, as dwb::child forms it
        down(wp, r, Ab);
        if (acc) down(wp, r, At);
        dwb::child(T, b, dof, B);
        dwb::m3v(B.R, ax, a);
        const float rate = dof[2 * (b - 1) + 1];
        for (int i = 0; i < 3; ++i) aq[i] = a[i] * rate;
        dwb::cross(wp, aq, c);
        joint(a, 0.0f, c, Ab);
        if (acc) joint(a, acc[5 + b], c, At);
        else At = Ab;
        if (e & DWB_PATH_OWNER) put(B, a, Ab, At, E + E_KS + b * KW, E + E_KIN + b * QW);
    }
}

// s R I R' (xx, yy, zz, xy, xz, yz) times v
DWB_HD void symv(const float *I, const float *v, float *o) {
    o[0] = I[0] * v[0] + I[3] * v[1] + I[4] * v[2];
    o[1] = I[3] * v[0] + I[1] * v[1] + I[5] * v[2];
    o[2] = I[4] * v[0] + I[5] * v[1] + I[2] * v[2];
}

// a record's f = w (cdd - g), cdd = xdd + alpha x d + omega x (omega x d), and n = Ib alpha + omega x (Ib omega)
DWB_HD void wrench(float w, const float *I, const float *d, const float *om, const float *al, const float *xdd, const float *g, float *f, float *n) {
    float t[3], u[3], s[3], Ia[3], Iw[3];
    dwb::cross(al, d, t);
    dwb::cross(om, d, u);
    dwb::cross(om, u, s);
    for (int i = 0; i < 3; ++i) f[i] = w * ((xdd[i] + t[i] + s[i]) - g[i]);
    symv(I, al, Ia);
    symv(I, om, Iw);
    dwb::cross(om, Iw, t);
    for (int i = 0; i < 3; ++i) n[i] = Ia[i] + t[i];
}

// record k to REC: COM offset, weight, and the pairs asked for; mass_scale: the env's [38] or NULL; g: the gravity vector
DWB_HD void record(const Tab &T, float *E, const float *mass_scale, const float *g, int what, int k) {
    float rec[dwj::RW], R[9], d[3];
    dwj::record_inertia(T, E + E_KS, mass_scale, k, rec);
    const int ik = T.inert(k), m = T.clampi(T.i(ik + 1), NM - 1);
    const float c[3] = {T.f(ik + 3), T.f(ik + 4), T.f(ik + 5)};
    dwb::quat_to_mat(E + E_KS + m * KW + K_Q, R);
    dwb::m3v(R, c, d);
    const float I[6] = {rec[4], rec[5], rec[6], rec[7], rec[8], rec[9]};
    const float *kin = E + E_KIN + m * QW;
    float *o = E + E_REC + k * RW;
    o[R_PC] = rec[1]; o[R_PC + 1] = rec[2]; o[R_PC + 2] = rec[3];
    o[R_W] = rec[0];
    if (what & W_BIAS) wrench(rec[0], I, d, kin + Q_W, kin + Q_AB, kin + Q_XB, g, o + R_FB, o + R_NB);
    if (what & W_TAU) wrench(rec[0], I, d, kin + Q_W, kin + Q_AT, kin + Q_XT, g, o + R_FT, o + R_NT);
    if (what & W_MOM) {
        float t[3];
        dwb::cross(kin + Q_W, d, t);
        for (int i = 0; i < 3; ++i) o[R_P + i] = rec[0] * (kin[Q_V + i] + t[i]);
        symv(I, kin + Q_W, o + R_L);
    }
}

// F += f, N += n + r x f
DWB_HD void sum6(const float *r, const float *f, const float *n, float *F, float *N) {
    float t[3];
    dwb::cross(r, f, t);
    for (int i = 0; i < 3; ++i) { F[i] += f[i]; N[i] += n[i] + t[i]; }
}

// moving body i: force, and moment about x_i (the base: about p_ref), of the records of its subtree, in the records' order, for every variant
// asked for; a joint's row of OUT is its axis dotted with the moment (tau: plus armature times qdd), the base's rows are force and moment.  The
// base also sums the momentum about p_ref, the mass and the first moment, and shifts the angular momentum to the centre of mass.
// arm: the env's [33] or NULL; acc: the env's nu_dot [39] (read for tau with an armature only)
DWB_HD void body_sum(const Tab &T, float *E, const float *arm, const float *acc, const float *g, int what, int i) {
    const float *ks = E + E_KS + i * KW, *x = i == 0 ? ks + K_A : ks + K_OFF;
    const float x0 = x[0], x1 = x[1], x2 = x[2];
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    float Fb[3] = {0.0f, 0.0f, 0.0f}, Nb[3] = {0.0f, 0.0f, 0.0f}, Fg[3] = {0.0f, 0.0f, 0.0f}, Ng[3] = {0.0f, 0.0f, 0.0f};
    float Ft[3] = {0.0f, 0.0f, 0.0f}, Nt[3] = {0.0f, 0.0f, 0.0f}, P[3] = {0.0f, 0.0f, 0.0f}, L[3] = {0.0f, 0.0f, 0.0f};
    float h[3] = {0.0f, 0.0f, 0.0f}, mc = 0.0f;
    const bool mom = (what & W_MOM) && i == 0;
    for (uint64_t left = (uint64_t)T.w[DWJ_T_SUB + 2 * i] | ((uint64_t)T.w[DWJ_T_SUB + 2 * i + 1] << 32); left != 0; left &= left - 1) {
        const int k = T.clampi(__builtin_ctzll(left), NI - 1);
        const float *rec = E + E_REC + k * RW;
        const float w = rec[R_W], r[3] = {rec[R_PC] - x0, rec[R_PC + 1] - x1, rec[R_PC + 2] - x2};
        if (what & W_BIAS) sum6(r, rec + R_FB, rec + R_NB, Fb, Nb);
        if (what & W_GRAV) {
            const float fg[3] = {w * (0.0f - g[0]), w * (0.0f - g[1]), w * (0.0f - g[2])};
            sum6(r, fg, zero, Fg, Ng);
        }
        if (what & W_TAU) sum6(r, rec + R_FT, rec + R_NT, Ft, Nt);
        if (mom) {
            sum6(r, rec + R_P, rec + R_L, P, L);
            mc += w;
            for (int c = 0; c < 3; ++c) h[c] += w * r[c];
        }
    }
    float *o = E + E_OUT;
    if (i == 0) {
        for (int c = 0; c < 3; ++c) {
            if (what & W_BIAS) { o[O_BIAS + c] = Fb[c]; o[O_BIAS + 3 + c] = Nb[c]; }
            if (what & W_GRAV) { o[O_GRAV + c] = Fg[c]; o[O_GRAV + 3 + c] = Ng[c]; }
            if (what & W_TAU) { o[O_TAU + c] = Ft[c]; o[O_TAU + 3 + c] = Nt[c]; }
        }
        if (mom) {
            // the COM's offset from p_ref is h / mass; L about the COM = L about p_ref - that offset x P
            const float cm[3] = {h[0] / mc, h[1] / mc, h[2] / mc};
            float t[3];
            dwb::cross(cm, P, t);
            for (int c = 0; c < 3; ++c) { o[O_MOM + c] = P[c]; o[O_MOM + 3 + c] = L[c] - t[c]; }
        }
    } else {
        const float a0 = ks[K_A], a1 = ks[K_A + 1], a2 = ks[K_A + 2];
        if (what & W_BIAS) o[O_BIAS + 5 + i] = a0 * Nb[0] + a1 * Nb[1] + a2 * Nb[2];
        if (what & W_GRAV) o[O_GRAV + 5 + i] = a0 * Ng[0] + a1 * Ng[1] + a2 * Ng[2];
        if (what & W_TAU) {
            float v = a0 * Nt[0] + a1 * Nt[1] + a2 * Nt[2];
            if (arm && acc) v += arm[i - 1] * acc[5 + i];
            o[O_TAU + 5 + i] = v;
        }
    }
}

}  // namespace dwn

#endif
