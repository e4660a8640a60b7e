// dw_contact.h -- one env's contact-consistent dynamics (include/dyros_contact_dynamics.h), written once for the HIP kernel of
// dw_contact_dynamics.hip and for a g++ build (tests/contact_dynamics_host.cpp), which the CPU tests hold against a float64 numpy restatement.
// The chain walk is dw_dynamics.h's (its KS words are dw_jacobian.h's, its KIN words hold every body's velocity and its acceleration at
// nu_dot = 0), the mass matrix dw_jacobian.h's, the factor and the sweeps dw_factor.h's.  An env's store is dw_factor.h's (and a tail), then PT
// (the contact points' offsets from the base), JD (Jd_c nu), Y (J_c's rows, then the rows of M^-1 J_c', solved in place) and A (J_c Y, then its
// factor: D on the diagonal, L below it).  KIN lies where the mass matrix's records go later, so the contacts' words are formed first.  KS stays
// to the end: J_c is not stored, its words are formed from KS and PT wherever they are read.  Behind KS the store holds x0 [R][NV] once M is
// factored, then, once x0 is solved, the small columns [m + R][AS]: the identity's for A^-1 and the right sides of A f = g.
// Pieces: contact_kin (PT and JD of one contact), jc_word, row_dot (a row of J_c times a vector, over the at most 17 columns the row can hold),
// a_word, ldl_one / ldl_scale (the dense factor's updates), sfwd_one / sscale_one / sback_one (the small sweeps' updates), g_word, accel_word.
// pack() is the host's table builder.
#ifndef DW_CONTACT_H
#define DW_CONTACT_H

#include "../../include/dyros_contact_dynamics.h"
#include "dw_dynamics.h"
#include "dw_factor.h"
#include "dw_jacobian.h"

namespace dwc {

using dwb::Tab;
constexpr int NV = DWC_NV, NM = dwl::NM, NB = dwl::NB, MAXK = DWC_MAX_CONTACTS, MAXM = DWC_MAX_ROWS, MAXR = DWC_MAX_RHS;
constexpr int AS = MAXM + 1;          // the stride of A's rows and of the small columns: odd
// x0 and the small columns go behind KS, which jc_word reads to the end; the small columns run past dw_factor.h's store into TAIL
constexpr int E_X0 = dwj::E_REC, E_S = E_X0 + MAXR * NV, S_END = E_S + (MAXM + MAXR) * AS, TAIL = S_END > dwl::ENV ? S_END - dwl::ENV : 0;
constexpr int E_PT = dwl::ENV + TAIL, E_JD = E_PT + 3 * MAXK, E_Y = E_JD + MAXM, E_A = E_Y + MAXM * NV, ENV = E_A + MAXM * AS + 1;
static_assert(NV == DWL_NV && DWC_NUM_BODIES == DWL_NUM_BODIES && DWC_NUM_DOF == DWL_NUM_DOF, "one robot");
static_assert(MAXM == MAXK * DWC_ROWS && MAXM == dwl::CAP, "the rows of J_c are one column batch of the solve");
static_assert(DWC_T_K == DWL_TABLE_WORDS && DWC_T_CONTACT == DWC_T_K + 1 && DWC_TABLE_WORDS == DWC_T_CONTACT + 4 * MAXK + 3, "the table's sections");
static_assert(ENV % 2 == 1 && AS % 2 == 1, "odd strides");
static_assert(dwn::E_KS == dwj::E_KS && dwn::E_KIN + dwn::NM * dwn::QW <= dwl::ENV, "the chain walk's words lie inside the factor's store");
static_assert(E_X0 >= dwj::E_KS + dwj::NM * dwj::KW && E_S <= dwl::E_H && S_END <= E_PT, "x0 stands between KS and H, the small columns end before PT");
static_assert(E_PT + 3 * MAXK < 0x10000, "a point's word fits jac_word's resolved row");

DWB_HD int groups(int n) { return (n + DWC_GROUP - 1) / DWC_GROUP; }
DWB_HD int count(const Tab &T) { return T.clampi(T.i(DWC_T_K), MAXK); }
DWB_HD int body(const Tab &T, int i) { return T.clampi(T.i(DWC_T_CONTACT + 4 * i), NM - 1); }

// contact i after the chain walk: its point's offset from the base, x_b + R_b pos, to PT; the point's classical acceleration xdd_b + alpha_b x r
// + omega_b x (omega_b x r), r = R_b pos, and alpha_b, both at nu_dot = 0, to JD
DWB_HD void contact_kin(const Tab &T, float *E, int i) {
    const int b = body(T, i);
    const float pos[3] = {T.f(DWC_T_CONTACT + 4 * i + 1), T.f(DWC_T_CONTACT + 4 * i + 2), T.f(DWC_T_CONTACT + 4 * i + 3)};
    const float *ks = E + dwn::E_KS + b * dwn::KW, *kin = E + dwn::E_KIN + b * dwn::QW;
    float R[9], r[3], t[3], u[3], s[3];
    dwb::quat_to_mat(ks + dwn::K_Q, R);
    dwb::m3v(R, pos, r);
    dwb::cross(kin + dwn::Q_AB, r, t);
    dwb::cross(kin + dwn::Q_W, r, u);
    dwb::cross(kin + dwn::Q_W, u, s);
    for (int c = 0; c < 3; ++c) {
        E[E_PT + 3 * i + c] = ks[dwn::K_OFF + c] + r[c];
        E[E_JD + 6 * i + c] = kin[dwn::Q_XB + c] + t[c] + s[c];
        E[E_JD + 6 * i + 3 + c] = kin[dwn::Q_AB + c];
    }
}

// word (r, c) of J_c by dw_jacobian.h's jac_word at the contact's point
DWB_HD float jc_word(const Tab &T, const float *E, int r, int c) {
    const int i = r / 6;
    return dwj::jac_word(T, E, body(T, i) | ((E_PT + 3 * i) << 8), r - 6 * i, c);
}

// row r of J_c times v [NV]: the six base columns, then the joints on the path to the row's body, ascending.  J_c is not kept: its words are
// formed again from KS and PT (the same bits), so that an env's store stays small
DWB_HD float row_dot(const Tab &T, const float *E, int r, const float *v) {
    const int i = r / 6, w = r - 6 * i, m = body(T, i), row = m | ((E_PT + 3 * i) << 8);
    float a = 0.0f;
    for (int k = 0; k < 6; ++k) a += dwj::jac_word(T, E, row, w, k) * v[k];
    for (uint64_t left = (uint64_t)T.w[DWJ_T_ANC + 2 * m] | ((uint64_t)T.w[DWJ_T_ANC + 2 * m + 1] << 32); left != 0; left &= left - 1) {
        const int k = 5 + T.clampi(__builtin_ctzll(left), NM - 1);
        a += dwj::jac_word(T, E, row, w, k) * v[k];
    }
    return a;
}

// word (r, c), r >= c, of A = J_c Y
DWB_HD float a_word(const Tab &T, const float *E, int r, int c) { return row_dot(T, E, r, E + E_Y + c * NV); }

// the dense factor A = L D L' in place, column j = 0 .. m - 2 after column: update (i, k), j < k <= i, A[i][k] -= (A[i][j] / A[j][j]) A[k][j].  It
// reads column j and writes elsewhere: a column's updates run in any order, or side by side.  Then ldl_scale for every word below the diagonal
DWB_HD void ldl_one(float *A, int j, int i, int k) { A[i * AS + k] = A[i * AS + k] - (A[i * AS + j] / A[j * AS + j]) * A[k * AS + j]; }
DWB_HD void ldl_scale(float *A, int i, int j) { A[i * AS + j] = A[i * AS + j] / A[j * AS + j]; }

// A g = g in place, g [m]: sfwd_one for columns 0 up to m - 2 (g[i] -= L[i][j] g[j], i > j), sscale_one for every word, sback_one for rows m - 1
// down to 1 (g[i] -= L[j][i] g[j], i < j).  A step's updates touch different words and read none that the step writes
DWB_HD void sfwd_one(const float *A, float *g, int j, int i) { g[i] -= A[i * AS + j] * g[j]; }
DWB_HD void sscale_one(const float *A, float *g, int i) { g[i] = g[i] / A[i * AS + i]; }
DWB_HD void sback_one(const float *A, float *g, int j, int i) { g[i] -= A[j * AS + i] * g[j]; }
DWB_HD void small_solve(const float *A, float *g, int m) {
    for (int j = 0; j < m - 1; ++j)
        for (int i = j + 1; i < m; ++i) sfwd_one(A, g, j, i);
    for (int i = 0; i < m; ++i) sscale_one(A, g, i);
    for (int j = m - 1; j >= 1; --j)
        for (int i = 0; i < j; ++i) sback_one(A, g, j, i);
}

// word i of the right side of A f = g: (gamma - Jd_c nu) - J_c x0, in that order; gamma: the env's [m] or NULL
DWB_HD float g_word(const Tab &T, const float *E, const float *gamma, const float *x0, int i) {
    return ((gamma ? gamma[i] : 0.0f) - E[E_JD + i]) - row_dot(T, E, i, x0);
}

// word k of nu_dot = x0 + Y f, the rows' products added in ascending order
DWB_HD float accel_word(const float *E, const float *x0, const float *f, int m, int k) {
    float v = x0[k];
    for (int i = 0; i < m; ++i) v += E[E_Y + i * NV + k] * f[i];
    return v;
}

// word (r, c) of a mirrored output from columns W [..][AS]: the column of the smaller index, the row of the larger
DWB_HD float mirror_word(const float *W, int r, int c) { return r < c ? W[r * AS + c] : W[c * AS + r]; }

// ---- host: the table from the model and the contacts (dwc_pack_table) ----
// who: the entry point the refusals name (dw_contact_inverse.h's and dw_stance_inverse.h's tables begin with this one)
inline int pack(const DwjModel *M, const DwcContacts *Cn, uint32_t *t, char *err, size_t errn, const char *who = "dwc_pack_table") {
    auto fail = [&](const char *msg, int idx) { snprintf(err, errn, "%s: %s (index %d)", who, msg, idx); return -1; };
    if (!M || !Cn || !t) return fail("a pointer is missing", 0);
    memset(t, 0, sizeof(uint32_t) * DWC_TABLE_WORDS);
    if (dwl::pack(M, t, err, errn, who) != 0) return -1;
    if (Cn->count < 1 || Cn->count > MAXK) return fail("count must be in 1..DWC_MAX_CONTACTS = 4", 0);
    t[DWC_T_K] = (uint32_t)Cn->count;
    for (int i = 0; i < Cn->count; ++i) {
        const int g = Cn->body[i];
        if (g < 0 || g >= NB) return fail("a body id is outside 0..37", i);
        const int b = M->body_moving[g];          // (dwb::pack has checked its range)
        for (int j = 0; j < i; ++j)
            if ((int)t[DWC_T_CONTACT + 4 * j] == b) return fail("two contacts on one moving body: their rows would be dependent", i);
        t[DWC_T_CONTACT + 4 * i] = (uint32_t)b;
        for (int c = 0; c < 3; ++c) {
            if (!isfinite(Cn->pos[i][c])) return fail("pos is not finite", i);
            memcpy(t + DWC_T_CONTACT + 4 * i + 1 + c, &Cn->pos[i][c], 4);
        }
    }
    return 0;
}

}  // namespace dwc

#endif
