// dw_contact_inverse.h -- one env's contact inverse dynamics (include/dyros_contact_inverse_dynamics.h), written once for the HIP kernel of
// dw_contact_inverse.hip and for a g++ build (tests/contact_inverse_dynamics_host.cpp), which the CPU tests hold against a float64 numpy
// restatement.  The chain walk, the records and the subtree sums are dw_dynamics.h's with the caller's nu_dot (its tau row is r), J_c's words
// dw_jacobian.h's jac_word at the contact's point, as dw_contact.h forms them.  Nothing here needs M or its factor.  An env's store is
// dw_dynamics.h's, then PT (the contact points' offsets from the base), G (J_b' W^-1 J_b, then its factor: D on the diagonal, L below it),
// Y (the right side r[0:6] - J_b' f_ref, solved in place), F (the wrenches) and FR (f_ref, zeros when the caller has none).  CA (J_c a + Jd_c
// nu) goes to the gravity row of dw_dynamics.h's OUT, which this launch never asks for.
// Pieces: contact_point (PT and CA of one contact), jc_word, g_word, ldl_one / ldl_scale and sfwd_one / sscale_one / sback_one (dw_contact.h's
// updates at G's stride), y_word, f_word, tauj_word.  The sums over the rows go contact by contact over a `mask` of the contacts that carry
// load, then over a contact's six rows: dwi_solve passes every contact, dwk_solve (dw_stance_inverse.h) each env's stance; with every
// contact on these are the plain sums over r = 0 .. m - 1, term for term.  pack() is the host's table builder.
#ifndef DW_CONTACT_INVERSE_H
#define DW_CONTACT_INVERSE_H

#include "../../include/dyros_contact_inverse_dynamics.h"
#include "dw_contact.h"
#include "dw_dynamics.h"
#include "dw_jacobian.h"

namespace dwi {

using dwb::Tab;
constexpr int NV = DWI_NV, NM = dwn::NM, NB = dwn::NB, ND = DWI_NUM_DOF, MAXK = DWI_MAX_CONTACTS, MAXM = DWI_MAX_ROWS;
constexpr int GN = 6, GS = GN + 1, GW = GN * (GN + 1) / 2;          // G's size, the stride of its rows (odd), its words on and below the diagonal
constexpr int E_PT = dwn::ENV, E_G = E_PT + 3 * MAXK, E_Y = E_G + GN * GS, E_F = E_Y + GN, E_FR = E_F + MAXM, ENV = E_FR + MAXM;
constexpr int E_TAU = dwn::E_OUT + dwn::O_TAU, E_CA = dwn::E_OUT + dwn::O_GRAV;
static_assert(NV == DWN_NV && DWI_NUM_BODIES == DWN_NUM_BODIES && ND == DWN_NUM_DOF && DWI_GROUP == DWN_GROUP && DWI_LANES == DWN_LANES, "one robot, one layout");
static_assert(MAXK == DWC_MAX_CONTACTS && MAXM == MAXK * DWI_ROWS && DWI_ROWS == DWC_ROWS, "dw_contact.h's contacts");
static_assert(DWI_T_K == DWN_TABLE_WORDS && DWI_T_CONTACT == DWI_T_K + 1 && DWI_T_W == DWI_T_CONTACT + 4 * MAXK && DWI_TABLE_WORDS == DWI_T_W + MAXM + 3,
              "the table's sections");
static_assert(DWI_TABLE_WORDS % 4 == 0 && ENV % 2 == 1 && GS % 2 == 1, "16-byte pieces, odd strides");
static_assert(MAXM <= NV && E_PT + 3 * MAXK < 0x10000, "CA fits a row of OUT, a point's word fits jac_word's resolved row");

DWB_HD int count(const Tab &T) { return T.clampi(T.i(DWI_T_K), MAXK); }
DWB_HD int body(const Tab &T, int i) { return T.clampi(T.i(DWI_T_CONTACT + 4 * i), NM - 1); }
DWB_HD float weight(const Tab &T, int r) { return T.f(DWI_T_W + r); }

// contact i after the chain walk: its point's offset from the base, x_b + R_b pos, to PT; the point's classical acceleration xdd_b + alpha_b x d
// + omega_b x (omega_b x d), d = R_b pos, and alpha_b, both under the caller's nu_dot, to CA (dwc::contact_kin's formula on the other words)
DWB_HD void contact_point(const Tab &T, float *E, int i) {
    const int b = body(T, i);
    const float pos[3] = {T.f(DWI_T_CONTACT + 4 * i + 1), T.f(DWI_T_CONTACT + 4 * i + 2), T.f(DWI_T_CONTACT + 4 * i + 3)};
    const float *ks = E + dwn::E_KS + b * dwn::KW, *kin = E + dwn::E_KIN + b * dwn::QW;
    float R[9], r[3], t[3], u[3], s[3];
    dwb::quat_to_mat(ks + dwn::K_Q, R);
    dwb::m3v(R, pos, r);
    dwb::cross(kin + dwn::Q_AT, r, t);
    dwb::cross(kin + dwn::Q_W, r, u);
    dwb::cross(kin + dwn::Q_W, u, s);
    for (int c = 0; c < 3; ++c) {
        E[E_PT + 3 * i + c] = ks[dwn::K_OFF + c] + r[c];
        E[E_CA + 6 * i + c] = kin[dwn::Q_XT + c] + t[c] + s[c];
        E[E_CA + 6 * i + 3 + c] = kin[dwn::Q_AT + c];
    }
}

// word (r, c) of J_c by dw_jacobian.h's jac_word at the contact's point: dwc::jc_word's bits
DWB_HD float jc_word(const Tab &T, const float *E, int r, int c) {
    const int i = r / 6;
    return dwj::jac_word(T, E, body(T, i) | ((E_PT + 3 * i) << 8), r - 6 * i, c);
}

// the contacts that carry load as a mask, bit i for contact i; dwi_solve's is full(K)
DWB_HD bool on(uint32_t mask, int i) { return ((mask >> i) & 1u) != 0u; }
DWB_HD uint32_t full(int K) { return (1u << K) - 1u; }

// word u = 0 .. 20 of G's lower triangle, (i, j) with i >= j, row after row: the rows of J_b of the active contacts, ascending
DWB_HD void g_word(const Tab &T, float *E, int K, uint32_t mask, int u) {
    const int i = u < 1 ? 0 : (u < 3 ? 1 : (u < 6 ? 2 : (u < 10 ? 3 : (u < 15 ? 4 : 5)))), j = u - i * (i + 1) / 2;
    float v = 0.0f;
    for (int c = 0; c < K; ++c) {
        if (!on(mask, c)) continue;
        for (int r = 6 * c; r < 6 * c + 6; ++r) v += (jc_word(T, E, r, i) / weight(T, r)) * jc_word(T, E, r, j);
    }
    E[E_G + i * GS + j] = v;
    E[E_G + j * GS + i] = v;
}

// dw_contact.h's dense factor and small sweeps at G's stride (the factor lives on and below the diagonal)
DWB_HD void ldl_one(float *G, int j, int i, int k) { G[i * GS + k] = G[i * GS + k] - (G[i * GS + j] / G[j * GS + j]) * G[k * GS + j]; }
DWB_HD void ldl_scale(float *G, int i, int j) { G[i * GS + j] = G[i * GS + j] / G[j * GS + j]; }
DWB_HD void sfwd_one(const float *G, float *g, int j, int i) { g[i] -= G[i * GS + j] * g[j]; }
DWB_HD void sscale_one(const float *G, float *g, int i) { g[i] = g[i] / G[i * GS + i]; }
DWB_HD void sback_one(const float *G, float *g, int j, int i) { g[i] -= G[j * GS + i] * g[j]; }

// word k of the right side of G y = r[0:6] - J_b' f_ref, in that order, over the active rows
DWB_HD void y_word(const Tab &T, float *E, int K, uint32_t mask, int k) {
    float s = 0.0f;
    for (int c = 0; c < K; ++c) {
        if (!on(mask, c)) continue;
        for (int r = 6 * c; r < 6 * c + 6; ++r) s += jc_word(T, E, r, k) * E[E_FR + r];
    }
    E[E_Y + k] = E[E_TAU + k] - s;
}

// word r of f = f_ref + W^-1 J_b y; +0.0 for a row of an inactive contact
DWB_HD void f_word(const Tab &T, float *E, uint32_t mask, int r) {
    if (!on(mask, r / 6)) {
        E[E_F + r] = 0.0f;
        return;
    }
    float s = 0.0f;
    for (int k = 0; k < GN; ++k) s += jc_word(T, E, r, k) * E[E_Y + k];
    E[E_F + r] = E[E_FR + r] + s / weight(T, r);
}

// tau_joint[j] = r[6 + j] - J_j' f: the active contacts that have joint j on their path, ascending
DWB_HD float tauj_word(const Tab &T, const float *E, int K, uint32_t mask, int j) {
    float s = 0.0f;
    for (int i = 0; i < K; ++i) {
        if (!on(mask, i)) continue;
        const int b = body(T, i);
        if (!dwj::bit(T, DWJ_T_ANC, b, j + 1)) continue;
        for (int w = 0; w < 6; ++w) s += dwj::jac_word(T, E, b | ((E_PT + 3 * i) << 8), w, 6 + j) * E[E_F + 6 * i + w];
    }
    return E[E_TAU + 6 + j] - s;
}

// ---- host ----
// one env's factor and sweeps after g_word and y_word (the kernel spreads each step's updates over a wave)
inline void factor_host(float *E) {
    float *G = E + E_G, *y = E + E_Y;
    for (int j = 0; j < GN - 1; ++j)
        for (int i = j + 1; i < GN; ++i)
            for (int k = j + 1; k <= i; ++k) ldl_one(G, j, i, k);
    for (int i = 0; i < GN; ++i)
        for (int j = 0; j < i; ++j) ldl_scale(G, i, j);
    for (int j = 0; j < GN - 1; ++j)
        for (int i = j + 1; i < GN; ++i) sfwd_one(G, y, j, i);
    for (int i = 0; i < GN; ++i) sscale_one(G, y, i);
    for (int j = GN - 1; j >= 1; --j)
        for (int i = 0; i < j; ++i) sback_one(G, y, j, i);
}

// one env's solve after g_word and y_word: an empty stance factors nothing; then f
inline void solve_host(const Tab &T, float *E, int K, uint32_t mask) {
    if (mask != 0u) factor_host(E);
    for (int r = 0; r < 6 * K; ++r) f_word(T, E, mask, r);
}

// the table from the model, the contacts and the weights (dwi_pack_table); who: the entry point the refusals name
inline int pack(const DwjModel *M, const DwcContacts *Cn, const float *weights, uint32_t *t, char *err, size_t errn, const char *who = "dwi_pack_table") {
    auto fail = [&](const char *msg, int idx) { snprintf(err, errn, "%s: %s (index %d)", who, msg, idx); return -1; };
    if (!M || !Cn || !t) return fail("a pointer is missing", 0);
    memset(t, 0, sizeof(uint32_t) * DWI_TABLE_WORDS);
    uint32_t c[DWC_TABLE_WORDS];
    if (dwc::pack(M, Cn, c, err, errn, who) != 0) return -1;
    memcpy(t, c, sizeof(uint32_t) * DWI_T_K);          // (dwl_pack_table's table begins with dwj_pack_table's)
    memcpy(t + DWI_T_K, c + DWC_T_K, sizeof(uint32_t) * (1 + 4 * MAXK));
    const float one = 1.0f;
    for (int r = 0; r < 6 * Cn->count; ++r) {
        if (weights && !(isfinite(weights[r]) && weights[r] > 0.0f)) return fail("a weight is not finite and positive", r);
        // one contact: J_b is square and f does not depend on W
        memcpy(t + DWI_T_W + r, weights && Cn->count > 1 ? weights + r : &one, 4);
    }
    return 0;
}

}  // namespace dwi

#endif
