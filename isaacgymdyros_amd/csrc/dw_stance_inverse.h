// dw_stance_inverse.h -- what one env's stance inverse dynamics (include/dyros_stance_inverse_dynamics.h) adds to dw_contact_inverse.h, for the
// HIP kernel of dw_contact_inverse.hip and for a g++ build (tests/contact_inverse_dynamics_host.cpp).  The arithmetic up to tau_joint, the
// sums over the active contacts included, is dw_contact_inverse.h's, and an env's store is its store.  Here: an env's `mask` from its stance
// bytes (bit i set when contact i carries load) and the new words base_word, margins4 and feasible_of.  pack() is the host's table builder.
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

using dwi::on;
// an env's mask from its K bytes of stance (NULL: every contact)
DWB_HD uint32_t mask_of(const uint8_t *stance, int K) {
    uint32_t mask = 0u;
    for (int i = 0; i < K; ++i) mask |= (stance == nullptr || stance[i] != 0) ? (1u << i) : 0u;
    return mask;
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
// the table from the model, the contacts, the weights, the soles and mu (dwk_pack_table)
inline int pack(const DwjModel *M, const DwcContacts *Cn, const float *weights, const float *soles, float mu, uint32_t *t, char *err, size_t errn) {
    auto fail = [&](const char *msg, int idx) { snprintf(err, errn, "dwk_pack_table: %s (index %d)", msg, idx); return -1; };
    if (!M || !Cn || !t) return fail("a pointer is missing", 0);
    memset(t, 0, sizeof(uint32_t) * DWK_TABLE_WORDS);
    if (dwi::pack(M, Cn, weights, t, err, errn, "dwk_pack_table") != 0) return -1;
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
