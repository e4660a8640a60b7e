// dw_factor.h -- one env's sparse factorisation and solve of the joint-space inertia (include/dyros_forward_dynamics.h), written once for the
// HIP kernel of dw_forward_dynamics.hip and for a g++ build (tests/forward_dynamics_host.cpp), which the CPU tests hold against a float64 numpy
// restatement.  The front end is dw_jacobian.h's (walk_path, record_inertia, body_sum, mm_word).  An env's pattern store H is DWL_PATTERN
// floats, the lower triangle's words that can be non-zero, row after row, a row's columns ascending and its diagonal last.  Because a row's
// columns are the base's six, the joints of its ancestors and itself, the columns of row k up to its word s are exactly the columns of row
// c_s: word (c_s, c_t) of the store is word t of row c_s.  Pieces: form_word (M into the store), eliminate_one (one update of a row's
// elimination), scale_word (a row's multipliers), back_one, scale_one, fwd_one (the updates of both triangular sweeps and the diagonal scaling),
// factor_word and minv_word (the outputs' words).  pack() is the host's table builder.
#ifndef DW_FACTOR_H
#define DW_FACTOR_H

#include "../../include/dyros_forward_dynamics.h"
#include "dw_jacobian.h"

namespace dwl {

using dwb::Tab;
constexpr int NV = DWL_NV, PAT = DWL_PATTERN, MAXROW = DWL_MAX_ROW, NM = DWL_NUM_MOVING, NB = DWL_NUM_BODIES, MMW = NV * NV;
// an env's store: dw_jacobian.h's mass-matrix store, then H.  Once M's words stand in H the first part is free, and holds CAP right-hand sides
constexpr int E_H = dwj::MM_ENV, ENV = E_H + PAT, CAP = dwj::MM_ENV / NV;
static_assert(NV == DWJ_NV && NM == DWJ_NUM_MOVING && NB == DWJ_NUM_BODIES && DWL_NUM_DOF == DWJ_NUM_DOF, "one robot");
constexpr int TPAT = PAT - NV;          // words below the diagonal
static_assert(DWL_T_ROW == DWJ_TABLE_WORDS && DWL_T_COL == DWL_T_ROW + NV + 1 && DWL_T_TROW == DWL_T_COL + PAT && DWL_T_TCOL == DWL_T_TROW + NV + 1 &&
                  DWL_TABLE_WORDS == DWL_T_TCOL + TPAT + 3,
              "the table's sections");
static_assert(ENV % 2 == 1 && NV % 2 == 1, "odd strides");
static_assert(MAXROW - 1 <= 16, "a row's updates are numbered s << 4 | t");
static_assert(2 * CAP >= NV + DWL_MAX_RHS, "two passes hold every column of a call");

DWB_HD int groups(int n) { return (n + DWL_GROUP - 1) / DWL_GROUP; }
// the first pattern word of row r (r = NV: the pattern's end), and a row's words, the diagonal included
DWB_HD int row_start(const Tab &T, int r) { return T.clampi(T.i(DWL_T_ROW + r), PAT); }
DWB_HD int clamp_len(int n) { return n < 0 ? 0 : (n > MAXROW ? MAXROW : n); }
DWB_HD int row_len(const Tab &T, int r) { return clamp_len(row_start(T, r + 1) - row_start(T, r)); }
DWB_HD int pat_col(const Tab &T, int p) { return T.clampi(T.i(DWL_T_COL + p) & 255, NV - 1); }
DWB_HD int pat_row(const Tab &T, int p) { return T.clampi(T.i(DWL_T_COL + p) >> 8, NV - 1); }
DWB_HD int tcol_start(const Tab &T, int c) { return T.clampi(T.i(DWL_T_TROW + c), TPAT); }
DWB_HD int at(int p) { return p < 0 ? 0 : (p > PAT - 1 ? PAT - 1 : p); }          // (a damaged table must not index past the store)

// pattern word p of M, by dw_jacobian.h's mm_word: the bits of dwj_mass_matrix.  E = the env's store after body_sum
DWB_HD float form_word(const Tab &T, const float *E, const float *arm, int p) { return dwj::mm_word(T, E, arm, pat_row(T, p), pat_col(T, p)); }

// row k's elimination, update (s, t), t <= s < n - 1, of the row that starts at word r0 and holds n words: M[c_s][c_t] -= (M[k][c_s] / M[k][k])
// M[k][c_t].  It reads row k and a word of a row above it, *p, and returns that word's new value: every (s, t) has another word, so the
// updates of a row run in any order, or side by side, all reads before all writes
DWB_HD float eliminate_one(const Tab &T, const float *H, int r0, int n, int s, int t, int *p) {
    const float a = H[at(r0 + s)] / H[at(r0 + n - 1)];
    *p = at(row_start(T, pat_col(T, at(r0 + s))) + t);
    return H[*p] - a * H[at(r0 + t)];
}

// after every row's elimination: pattern word p below the diagonal becomes its multiplier, L[k][c_s] = M[k][c_s] / D[k]; the diagonal stays
DWB_HD void scale_word(const Tab &T, float *H, int p) {
    const int r = pat_row(T, p);
    if (pat_col(T, p) < r) H[p] = H[p] / H[at(row_start(T, r + 1) - 1)];
}

// The solve of one right-hand side b [NV] in place, b -> M^-1 b = L^-1 D^-1 L'^-1 b, as steps of independent updates over the pattern of the
// factored store: back_one for rows 38 down to 1 (row k's words: b[c_s] -= L[k][c_s] b[k]), scale_one for every word (b[k] /= D[k]), fwd_one for
// columns 0 up to 37 (column i's words: b[k] -= L[k][i] b[i]; a word b[k] so receives its row's products in ascending column order).  The
// updates of one step touch different words and read none that the step writes: they run in any order, or side by side
DWB_HD void back_one(const Tab &T, const float *H, float *b, int k, int r0, int s) {
    const int p = at(r0 + s);
    b[pat_col(T, p)] -= H[p] * b[k];
}
DWB_HD void scale_one(const Tab &T, const float *H, float *b, int k) { b[k] = b[k] / H[at(row_start(T, k + 1) - 1)]; }
DWB_HD void fwd_one(const Tab &T, const float *H, float *b, int i, int q0, int j) {
    const int q = q0 + j, w = T.i(DWL_T_TCOL + (q < 0 ? 0 : (q > TPAT - 1 ? TPAT - 1 : q)));
    b[T.clampi(w >> 16, NV - 1)] -= H[at(w & 0xffff)] * b[i];
}
// the three sweeps of one right-hand side, step after step (the kernel runs the steps of its columns side by side)
DWB_HD void solve_column(const Tab &T, const float *H, float *b) {
    for (int k = NV - 1; k >= 1; --k)
        for (int s = 0; s < row_len(T, k) - 1; ++s) back_one(T, H, b, k, row_start(T, k), s);
    for (int k = 0; k < NV; ++k) scale_one(T, H, b, k);
    for (int i = 0; i < NV - 1; ++i)
        for (int j = 0; j < tcol_start(T, i + 1) - tcol_start(T, i); ++j) fwd_one(T, H, b, i, tcol_start(T, i), j);
}

// word (r, c) of the factor output: the store's word inside the pattern, +0.0 above the diagonal and outside the pattern
DWB_HD float factor_word(const Tab &T, const float *H, int r, int c) {
    if (c > r) return 0.0f;
    if (c < 6) return H[at(row_start(T, r) + c)];
    const int m = r - 5, b = c - 5;          // (c >= 6: r >= 6 too)
    if (!dwj::bit(T, DWJ_T_ANC, m, b)) return 0.0f;
    const uint64_t anc = (uint64_t)T.w[DWJ_T_ANC + 2 * m] | ((uint64_t)T.w[DWJ_T_ANC + 2 * m + 1] << 32);
    return H[at(row_start(T, r) + 6 + __builtin_popcountll(anc & ((1ull << b) - 1ull)))];
}

// word (r, c) of M^-1 from solved identity columns W [..][NV], which holds columns c0 .. c0 + nc - 1: the column of the smaller index, the row
// of the larger.  false: the word belongs to another pass
DWB_HD bool minv_word(const float *W, int c0, int nc, int r, int c, float *out) {
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    if (lo < c0 || lo >= c0 + nc) return false;
    *out = W[(lo - c0) * NV + hi];
    return true;
}

// ---- host: the table from the model (dwl_pack_table) ----
// who: the entry point the refusals name
inline int pack(const DwjModel *M, uint32_t *t, char *err, size_t errn, const char *who = "dwl_pack_table") {
    if (!M || !t) { snprintf(err, errn, "%s: a pointer is missing (index 0)", who); return -1; }
    memset(t, 0, sizeof(uint32_t) * DWL_TABLE_WORDS);
    if (dwj::pack(M, t, err, errn, who) != 0) return -1;
    // dwb::pack has checked that parents precede children: a row's ancestors ascend from the base's side
    int p = 0;
    for (int r = 0; r < NV; ++r) {
        t[DWL_T_ROW + r] = (uint32_t)p;
        int cols[NM + 6], n = 0;
        for (int c = 0; c < 6 && c < r; ++c) cols[n++] = c;
        if (r >= 6) {
            int anc[NM], na = 0;
            for (int b = M->mv_parent[r - 5]; b > 0; b = M->mv_parent[b]) anc[na++] = b;
            while (na > 0) cols[n++] = 5 + anc[--na];
        }
        cols[n++] = r;
        if (n > MAXROW) { snprintf(err, errn, "%s: a row of the pattern holds more than DWL_MAX_ROW words (index %d)", who, r); return -1; }
        if (p + n > PAT) { snprintf(err, errn, "%s: the pattern holds more than DWL_PATTERN words (index %d)", who, r); return -1; }
        for (int i = 0; i < n; ++i) t[DWL_T_COL + p++] = (uint32_t)((r << 8) | cols[i]);
    }
    t[DWL_T_ROW + NV] = (uint32_t)p;
    if (p != PAT) { snprintf(err, errn, "%s: the pattern holds %d words, not DWL_PATTERN (index 0)", who, p); return -1; }
    // the same words by columns, the diagonal left out
    int q = 0;
    for (int c = 0; c < NV; ++c) {
        t[DWL_T_TROW + c] = (uint32_t)q;
        for (int w = 0; w < PAT; ++w) {
            const int r = (int)(t[DWL_T_COL + w] >> 8);
            if ((int)(t[DWL_T_COL + w] & 255u) == c && r > c) t[DWL_T_TCOL + q++] = (uint32_t)((r << 16) | w);
        }
    }
    t[DWL_T_TROW + NV] = (uint32_t)q;
    return 0;
}

}  // namespace dwl

#endif
