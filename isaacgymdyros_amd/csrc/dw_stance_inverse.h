// dw_stance_inverse.h -- one env's stance inverse dynamics (include/dyros_stance_inverse_dynamics.h), written once for the HIP kernel of
// dw_stance_inverse.hip and for a g++ build (tests/stance_inverse_dynamics_host.cpp), which the CPU tests hold against a float64 numpy
// restatement.  The chain walk, the records, the subtree sums, the contact points, J_c's words, the factor and the sweeps are
// dw_contact_inverse.h's, and an env's store is its store; what is here are the sums over the rows, which visit the active contacts only
// (`mask`: bit i set when contact i carries load), and the new words: base_word, margins4, feasible_of.  pack() is the host's table builder.
#ifndef DW_STANCE_INVERSE_H
#define DW_STANCE_INVERSE_H

#include "../../include/dyros_stance_inverse_dynamics.h"
#include "dw_contact_inverse.h"

namespace dwk {

using dwb::Tab;
constexpr int NV = DWK_NV, ND = DWK_NUM_DOF, MAXK = DWK_MAX_CONTACTS, MAXM = DWK_MAX_ROWS, SW = DWK_SOLE_WORDS, MW = DWK_MARGINS;
static_assert(NV == DWI_NV && DWK_NUM_BODIES == DWI_NUM_BODIES && ND == DWI_NUM_DOF && DWK_GROUP == DWI_GROUP && DWK_LANES == DWI_LANES, "one robot, one layout");
static_assert(MAXK == DWI_MAX_CONTACTS && MAXM == DWI_MAX_ROWS && DWK_ROWS == DWI_ROWS, "dw_contact_inverse.h's contacts");
static_assert(DWK_T_SOLE == DWI_TABLE_WORDS && DWK_T_MU == DWK_T_SOLE + SW * MAXK && DWK_TABLE_WORDS == DWK_T_MU + 1 + 3 && DWK_TABLE_WORDS % 4 == 0,
              "the table's sections, 16-byte pieces");

DWB_HD bool on(uint32_t mask, int i) { return ((mask >> i) & 1u) != 0u; }
// an env's mask from its K bytes of stance (NULL: every contact)
DWB_HD uint32_t mask_of(const uint8_t *stance, int K) {
    uint32_t mask = 0u;
    for (int i = 0; i < K; ++i) mask |= (stance == nullptr || stance[i] != 0) ? (1u << i) : 0u;
    return mask;
}

// dwi::g_word over the active rows
DWB_HD void g_word(const Tab &T, float *E, int K, uint32_t mask, int u) {
    const int i = u < 1 ? 0 : (u < 3 ? 1 : (u < 6 ? 2 : (u < 10 ? 3 : (u < 15 ? 4 : 5)))), j = u - i * (i + 1) / 2;
    float v = 0.0f;
    for (int c = 0; c < K; ++c) {
        if (!on(mask, c)) continue;
        for (int r = 6 * c; r < 6 * c + 6; ++r) v += (dwi::jc_word(T, E, r, i) / dwi::weight(T, r)) * dwi::jc_word(T, E, r, j);
    }
    E[dwi::E_G + i * dwi::GS + j] = v;
    E[dwi::E_G + j * dwi::GS + i] = v;
}

// dwi::y_word over the active rows
DWB_HD void y_word(const Tab &T, float *E, int K, uint32_t mask, int k) {
    float s = 0.0f;
    for (int c = 0; c < K; ++c) {
        if (!on(mask, c)) continue;
        for (int r = 6 * c; r < 6 * c + 6; ++r) s += dwi::jc_word(T, E, r, k) * E[dwi::E_FR + r];
    }
    E[dwi::E_Y + k] = E[dwi::E_TAU + k] - s;
}

// word r of f: dwi::f_word for an active row, +0.0 for an inactive one
DWB_HD void f_word(const Tab &T, float *E, uint32_t mask, int r) {
    if (on(mask, r / 6)) dwi::f_word(T, E, r);
    else E[dwi::E_F + r] = 0.0f;
}

// dwi::tauj_word over the active contacts
DWB_HD float tauj_word(const Tab &T, const float *E, int K, uint32_t mask, int j) {
    float s = 0.0f;
    for (int i = 0; i < K; ++i) {
        if (!on(mask, i)) continue;
        const int b = dwi::body(T, i);
        if (!dwj::bit(T, DWJ_T_ANC, b, j + 1)) continue;
        for (int w = 0; w < 6; ++w) s += dwj::jac_word(T, E, b | ((dwi::E_PT + 3 * i) << 8), w, 6 + j) * E[dwi::E_F + 6 * i + w];
    }
    return E[dwi::E_TAU + 6 + j] - s;
}

// base_residual[k] = r[k] - J_b' f over the active rows, ascending
DWB_HD float base_word(const Tab &T, const float *E, int K, uint32_t mask, int k) {
    float s = 0.0f;
    for (int c = 0; c < K; ++c) {
        if (!on(mask, c)) continue;
        for (int r = 6 * c; r < 6 * c + 6; ++r) s += dwi::jc_word(T, E, r, k) * E[dwi::E_F + r];
    }
    return E[dwi::E_TAU + k] - s;
}

// the four margins of contact i from its wrench in F, in the header's order; +0.0 for an inactive contact
DWB_HD void margins4(const Tab &T, const float *E, uint32_t mask, int i, float *o) {
    if (!on(mask, i)) {
        o[0] = o[1] = o[2] = o[3] = 0.0f;
        return;
    }
    const float *ks = E + dwn::E_KS + dwi::body(T, i) * dwn::KW, *f = E + dwi::E_F + 6 * i, *m = f + 3;
    const int so = DWK_T_SOLE + SW * i;
    const float mu = T.f(DWK_T_MU), hx = T.f(so + 3), hy = T.f(so + 4);
    float R[9], fb[3], mb[3], d[3];
    dwb::quat_to_mat(ks + dwn::K_Q, R);
    for (int c = 0; c < 3; ++c) {
        fb[c] = R[c] * f[0] + R[3 + c] * f[1] + R[6 + c] * f[2];
        mb[c] = R[c] * m[0] + R[3 + c] * m[1] + R[6 + c] * m[2];
        d[c] = T.f(so + c) - T.f(DWI_T_CONTACT + 4 * i + 1 + c);
    }
    const float msx = mb[0] - (d[1] * fb[2] - d[2] * fb[1]), msy = mb[1] - (d[2] * fb[0] - d[0] * fb[2]);
    o[0] = fb[2];
    o[1] = mu * fb[2] - sqrtf(fb[0] * fb[0] + fb[1] * fb[1]);
    o[2] = hx * fb[2] - fabsf(msy);
    o[3] = hy * fb[2] - fabsf(msx);
}

// 1 when the stance is not empty and every margin of every active contact is >= 0 (a NaN is not)
DWB_HD uint8_t feasible_of(const Tab &T, const float *E, int K, uint32_t mask) {
    bool ok = mask != 0u;
    for (int i = 0; i < K; ++i) {
        if (!on(mask, i)) continue;
        float o[4];
        margins4(T, E, mask, i, o);
        ok = ok && o[0] >= 0.0f && o[1] >= 0.0f && o[2] >= 0.0f && o[3] >= 0.0f;
    }
    return ok ? 1 : 0;
}

// ---- host ----
// one env's solve after g_word and y_word (the kernel spreads each step's updates over a wave); an empty stance factors nothing
inline void solve_host(const Tab &T, float *E, int K, uint32_t mask) {
    if (mask != 0u) {
        float *G = E + dwi::E_G, *y = E + dwi::E_Y;
        for (int j = 0; j < dwi::GN - 1; ++j)
            for (int i = j + 1; i < dwi::GN; ++i)
                for (int k = j + 1; k <= i; ++k) dwi::ldl_one(G, j, i, k);
        for (int i = 0; i < dwi::GN; ++i)
            for (int j = 0; j < i; ++j) dwi::ldl_scale(G, i, j);
        for (int j = 0; j < dwi::GN - 1; ++j)
            for (int i = j + 1; i < dwi::GN; ++i) dwi::sfwd_one(G, y, j, i);
        for (int i = 0; i < dwi::GN; ++i) dwi::sscale_one(G, y, i);
        for (int j = dwi::GN - 1; j >= 1; --j)
            for (int i = 0; i < j; ++i) dwi::sback_one(G, y, j, i);
    }
    for (int r = 0; r < 6 * K; ++r) f_word(T, E, mask, r);
}

// the table from the model, the contacts, the weights, the soles and mu (dwk_pack_table)
inline int pack(const DwjModel *M, const DwcContacts *Cn, const float *weights, const float *soles, float mu, uint32_t *t, char *err, size_t errn) {
    auto fail = [&](const char *msg, int idx) { snprintf(err, errn, "dwk_pack_table: %s (index %d)", msg, idx); return -1; };
    if (!M || !Cn || !t) return fail("a pointer is missing", 0);
    memset(t, 0, sizeof(uint32_t) * DWK_TABLE_WORDS);
    if (dwi::pack(M, Cn, weights, t, err, errn) != 0) {
        if (errn > 2 && err[0] == 'd' && err[1] == 'w' && err[2] == 'i') err[2] = 'k';          // (the refusal is this entry point's)
        return -1;
    }
    for (int i = 0; i < Cn->count; ++i)
        for (int c = 0; c < SW; ++c) {
            // no sole: a point at the contact's pos
            const float v = soles ? soles[SW * i + c] : (c < 3 ? Cn->pos[i][c] : 0.0f);
            if (!isfinite(v)) return fail("a sole is not finite", i);
            if (c >= 3 && v < 0.0f) return fail("a half extent of a sole is negative", i);
            memcpy(t + DWK_T_SOLE + SW * i + c, &v, 4);
        }
    if (!(isfinite(mu) && mu > 0.0f)) return fail("mu is not finite and positive", 0);
    memcpy(t + DWK_T_MU, &mu, 4);
    return 0;
}

}  // namespace dwk

#endif
