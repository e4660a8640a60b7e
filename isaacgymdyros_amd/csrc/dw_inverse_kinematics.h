// dw_inverse_kinematics.h -- one env's inverse kinematics (include/dyros_inverse_kinematics.h), written once for the HIP kernel of
// dw_inverse_kinematics.hip and for a g++ build (tests/inverse_kinematics_host.cpp), which the CPU tests hold against a float64 numpy
// restatement.  The chain walk is dw_jacobian.h's walk_path at vel_at_com = 0 (its KS words: every moving body's offset from the base,
// quaternion and world joint axis), J's words its jac_word at the targets' points, as dw_contact.h forms them; the dense factor and the
// sweeps are dw_contact.h's functions at its stride.  The iterate is not kept here: it lives in the caller's copies of the env's root row
// [13] and dof_state row [33][2], which the walk reads unchanged.  An env's store is KS, then PT (the points' offsets from the base), ERR
// (the error rows), J [m][NV], A [m][AS] (J J' + lambda^2 W^-1, then its factor: D on the diagonal, L below it), Y (the right side, solved
// in place), DV (J' y) and three words of state: DEAD, DONE (0 or 1) and ITERS (the updates applied, a small whole number).
// Pieces, each one word or one row so that the kernel gives them a lane each: point, err_row, status, j_word, a_word, dv_word, step_scale,
// update_joint, update_base, err_max.  solve_host is the whole loop in the kernel's order; pack() is the host's table builder.
#ifndef DW_INVERSE_KINEMATICS_H
#define DW_INVERSE_KINEMATICS_H

#include "../../include/dyros_inverse_kinematics.h"
#include "dw_contact.h"
#include "dw_jacobian.h"

namespace dwq {

using dwb::Tab;
constexpr int NV = DWQ_NV, NM = dwj::NM, NB = dwj::NB, ND = DWQ_NUM_DOF, MAXK = DWQ_MAX_TARGETS, MAXM = DWQ_MAX_ROWS, TW = 7;
constexpr int AS = dwc::AS;          // the stride of A's rows: dw_contact.h's, odd
constexpr int E_PT = dwj::E_KS + NM * dwj::KW, E_ERR = E_PT + 3 * MAXK, E_J = E_ERR + MAXM, E_A = E_J + MAXM * NV, E_Y = E_A + MAXM * AS,
              E_DV = E_Y + MAXM, E_DEAD = E_DV + NV, E_DONE = E_DEAD + 1, E_ITERS = E_DONE + 1, ENV = E_ITERS + 2;
static_assert(NV == DWJ_NV && DWQ_NUM_BODIES == DWJ_NUM_BODIES && ND == DWJ_NUM_DOF, "one robot");
static_assert(MAXK == DWC_MAX_CONTACTS && MAXM == MAXK * DWQ_ROWS && DWQ_ROWS == DWC_ROWS && MAXM == DWC_MAX_ROWS, "dw_contact.h's contacts and its factor");
static_assert(DWQ_T_K == DWJ_TABLE_WORDS && DWQ_T_TARGET == DWQ_T_K + 1 && DWQ_T_ROWS == DWQ_T_TARGET + 4 * MAXK && DWQ_T_W == DWQ_T_ROWS + 1 &&
              DWQ_T_DOFS == DWQ_T_W + MAXM && DWQ_T_LIMIT == DWQ_T_DOFS + 2 && DWQ_T_PARAM == DWQ_T_LIMIT + 2 * ND && DWQ_TABLE_WORDS == DWQ_T_PARAM + 6,
              "the table's sections");
static_assert(DWQ_TABLE_WORDS % 4 == 0 && ENV % 2 == 1 && AS % 2 == 1 && NV % 2 == 1, "16-byte pieces, odd strides");
static_assert(E_PT + 3 * MAXK < 0x10000 && MAXM % 2 == 0, "a point's word fits jac_word's resolved row; A's triangle folds into m / 2 rows of m + 1 words");

DWB_HD int groups(int n) { return (n + DWQ_GROUP - 1) / DWQ_GROUP; }
DWB_HD int count(const Tab &T) { return T.clampi(T.i(DWQ_T_K), MAXK); }
DWB_HD int body(const Tab &T, int i) { return T.clampi(T.i(DWQ_T_TARGET + 4 * i), NM - 1); }
DWB_HD bool row_on(const Tab &T, int r) { return ((T.w[DWQ_T_ROWS] >> r) & 1u) != 0u; }
DWB_HD bool dof_on(const Tab &T, int j) { return ((T.w[DWQ_T_DOFS + (j >> 5)] >> (j & 31)) & 1u) != 0u; }
DWB_HD float weight(const Tab &T, int r) { return T.f(DWQ_T_W + r); }
DWB_HD int iterations(const Tab &T) { return T.clampi(T.i(DWQ_T_PARAM), DWQ_MAX_ITERATIONS); }
DWB_HD float damping(const Tab &T) { return T.f(DWQ_T_PARAM + 1); }
DWB_HD float max_step(const Tab &T) { return T.f(DWQ_T_PARAM + 2); }
DWB_HD float tol(const Tab &T, int r) { return T.f(DWQ_T_PARAM + (r % 6 < 3 ? 3 : 4)); }
DWB_HD bool flag(const Tab &T, int f) { return (T.i(DWQ_T_PARAM + 5) & f) != 0; }
// column c of J is free to move: a base column with a free base, a joint column inside the DoF mask
DWB_HD bool col_on(const Tab &T, int c) { return c < 6 ? flag(T, DWQ_F_FREE_BASE) : dof_on(T, c - 6); }

// target i after the chain walk: its point's offset from the base, x_b + R_b pos, to PT
DWB_HD void point(const Tab &T, float *E, int i) {
    const float pos[3] = {T.f(DWQ_T_TARGET + 4 * i + 1), T.f(DWQ_T_TARGET + 4 * i + 2), T.f(DWQ_T_TARGET + 4 * i + 3)};
    const float *ks = E + dwj::E_KS + body(T, i) * dwj::KW;
    float R[9], r[3];
    dwb::quat_to_mat(ks + dwj::K_Q, R);
    dwb::m3v(R, pos, r);
    for (int c = 0; c < 3; ++c) E[E_PT + 3 * i + c] = ks[dwj::K_OFF + c] + r[c];
}

// the squared norm's root of target i's quaternion as the caller gave it; tgt: the env's [K][7]
DWB_HD float target_norm(const float *tgt, int i) {
    const float *q = tgt + TW * i + 3;
    return sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
}

// error row r after point(): position rows (t_pos - base_pos) - PT, the first difference first (with targets_rel_root: t_pos - PT);
// orientation rows 2 sign(w) v of q_target (x) conj(q_body), the target normalised here; an inactive row +0.0.  root: the env's row [13]
DWB_HD void err_row(const Tab &T, float *E, const float *root, const float *tgt, int r) {
    const int i = r / 6, w = r - 6 * i;
    float e = 0.0f;
    if (row_on(T, r)) {
        if (w < 3) {
            const float t = tgt[TW * i + w];
            e = (flag(T, DWQ_F_REL_ROOT) ? t : t - root[w]) - E[E_PT + 3 * i + w];
        } else {
            const float n = target_norm(tgt, i);
            const float *qb = E + dwj::E_KS + body(T, i) * dwj::KW + dwj::K_Q;
            const float qt[4] = {tgt[TW * i + 3] / n, tgt[TW * i + 4] / n, tgt[TW * i + 5] / n, tgt[TW * i + 6] / n};
            const float qc[4] = {-qb[0], -qb[1], -qb[2], qb[3]};
            float qe[4];
            dwb::quat_mul(qt, qc, qe);
            const float v = w == 3 ? qe[0] : (w == 4 ? qe[1] : qe[2]);          // (no run-time index into a local array)
            e = 2.0f * (qe[3] < 0.0f ? -v : v);
        }
    }
    E[E_ERR + r] = e;
}

// after the error rows: DEAD (sticky) where a target's quaternion has a norm outside [0.99, 1.01] or an error word is not finite; DONE where
// every active row is within its tolerance
DWB_HD void status(const Tab &T, float *E, const float *tgt, int K) {
    bool dead = E[E_DEAD] != 0.0f, done = true;
    for (int i = 0; i < K; ++i) {
        const float n = target_norm(tgt, i);
        if (!(n >= 0.99f && n <= 1.01f)) dead = true;
    }
    for (int r = 0; r < 6 * K; ++r) {
        const float a = fabsf(E[E_ERR + r]);
        if (!(a <= 3.0e38f)) dead = true;
        if (row_on(T, r) && !(a <= tol(T, r))) done = false;
    }
    E[E_DEAD] = dead ? 1.0f : 0.0f;
    E[E_DONE] = done && !dead ? 1.0f : 0.0f;
}
// the env takes this iteration's update
DWB_HD bool moving(const float *E) { return E[E_DEAD] == 0.0f && E[E_DONE] == 0.0f; }

// word (r, c) of J: dw_jacobian.h's jac_word at the target's point; +0.0 in an inactive row and in a column that is held
DWB_HD void j_word(const Tab &T, float *E, int r, int c) {
    const int i = r / 6;
    E[E_J + r * NV + c] = row_on(T, r) && col_on(T, c) ? dwj::jac_word(T, E, body(T, i) | ((E_PT + 3 * i) << 8), r - 6 * i, c) : 0.0f;
}

// word u = 0 .. m (m + 1) / 2 - 1 of A's lower triangle, folded: u = a (m + 1) + b, a < m / 2; b <= a is (a, b), otherwise (m - 1 - a,
// b - a - 1).  A[i][j] = sum over c ascending of J[i][c] J[j][c], the diagonal + lambda lambda / w_i; an inactive row's diagonal is 1
DWB_HD void a_word(const Tab &T, float *E, int m, int u) {
    const int a = u / (m + 1), b = u - a * (m + 1);
    const int i = b <= a ? a : m - 1 - a, j = b <= a ? b : b - a - 1;
    const float *Ji = E + E_J + i * NV, *Jj = E + E_J + j * NV;
    float v = 0.0f;
    for (int c = 0; c < NV; ++c) v += Ji[c] * Jj[c];
    if (i == j) v = row_on(T, i) ? v + (damping(T) * damping(T)) / weight(T, i) : 1.0f;
    E[E_A + i * AS + j] = v;
    E[E_A + j * AS + i] = v;
}

// word c of dnu = J' y, the rows ascending
DWB_HD void dv_word(float *E, int m, int c) {
    float s = 0.0f;
    for (int r = 0; r < m; ++r) s += E[E_J + r * NV + c] * E[E_Y + r];
    E[E_DV + c] = s;
}

// the step limit's factor: max_step / max_j |dnu[6 + j]| where that exceeds max_step, else 1
DWB_HD float step_scale(const Tab &T, const float *E) {
    float big = 0.0f;
    for (int j = 0; j < ND; ++j) {
        const float a = fabsf(E[E_DV + 6 + j]);
        big = a > big ? a : big;
    }
    const float lim = max_step(T);
    return big > lim ? lim / big : 1.0f;
}

// joint j's update in the env's dof_state row: only a masked joint is touched
DWB_HD void update_joint(const Tab &T, const float *E, float *dof, int j, float s) {
    if (!dof_on(T, j)) return;
    float q = dof[2 * j] + E[E_DV + 6 + j] * s;
    if (flag(T, DWQ_F_CLAMP)) {
        const float lo = T.f(DWQ_T_LIMIT + 2 * j), hi = T.f(DWQ_T_LIMIT + 2 * j + 1);
        q = q < lo ? lo : (q > hi ? hi : q);
    }
    dof[2 * j] = q;
}

// the base's update in the env's root row: x += dnu[0:3], quat = normalise((dnu[3:6] / 2, 1) (x) quat), the quaternion normalised first as
// the walk reads it
DWB_HD void update_base(const float *E, float *root, float s) {
    const float n = sqrtf(root[3] * root[3] + root[4] * root[4] + root[5] * root[5] + root[6] * root[6]);
    const float q[4] = {root[3] / n, root[4] / n, root[5] / n, root[6] / n};
    const float d[4] = {0.5f * (E[E_DV + 3] * s), 0.5f * (E[E_DV + 4] * s), 0.5f * (E[E_DV + 5] * s), 1.0f};
    float o[4];
    dwb::quat_mul(d, q, o);
    const float k = sqrtf(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
    for (int c = 0; c < 3; ++c) root[c] = root[c] + E[E_DV + c] * s;
    for (int c = 0; c < 4; ++c) root[3 + c] = o[c] / k;
}

// word h of err [2]: the largest |e| over the active position rows (h = 0), orientation rows (h = 1); +0.0 with none
DWB_HD float err_max(const Tab &T, const float *E, int K, int h) {
    float big = 0.0f;
    for (int r = 0; r < 6 * K; ++r) {
        const float a = fabsf(E[E_ERR + r]);
        if (row_on(T, r) && (r % 6 >= 3) == (h != 0) && a > big) big = a;
    }
    return big;
}

// ---- host ----
// the walk, the points, the error rows and the status of one env, as the kernel orders them
inline void look(const Tab &T, float *E, const float *root, const float *dof, const float *tgt, int K) {
    for (int l = 0; l < T.nleaf(); ++l) dwj::walk_path(T, l, root, dof, 0, E + dwj::E_KS);
    for (int i = 0; i < K; ++i) point(T, E, i);
    for (int r = 0; r < 6 * K; ++r) err_row(T, E, root, tgt, r);
    status(T, E, tgt, K);
}

// one env's whole solve: root [13] and dof [33][2] are the caller's copies and hold the iterate; E [ENV] ends with the final error rows
inline void solve_host(const Tab &T, float *E, float *root, float *dof, const float *tgt) {
    const int K = count(T), m = 6 * K, I = iterations(T);
    memset(E, 0, sizeof(float) * ENV);
    for (int it = 0; it < I; ++it) {
        look(T, E, root, dof, tgt, K);
        if (!moving(E)) continue;
        for (int r = 0; r < m; ++r)
            for (int c = 0; c < NV; ++c) j_word(T, E, r, c);
        for (int u = 0; u < m / 2 * (m + 1); ++u) a_word(T, E, m, u);
        for (int r = 0; r < m; ++r) E[E_Y + r] = E[E_ERR + r];
        float *A = E + E_A;
        for (int j = 0; j < m - 1; ++j)
            for (int i = j + 1; i < m; ++i)
                for (int k = j + 1; k <= i; ++k) dwc::ldl_one(A, j, i, k);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < i; ++j) dwc::ldl_scale(A, i, j);
        dwc::small_solve(A, E + E_Y, m);
        for (int c = 0; c < NV; ++c) dv_word(E, m, c);
        const float s = step_scale(T, E);
        for (int j = 0; j < ND; ++j) update_joint(T, E, dof, j, s);
        if (flag(T, DWQ_F_FREE_BASE)) update_base(E, root, s);
        E[E_ITERS] += 1.0f;
    }
    look(T, E, root, dof, tgt, K);
}

// the table from the model, the targets and the solver's settings (dwq_pack_table); who: the entry point the refusals name
inline int pack(const DwjModel *M, const DwcContacts *Tg, const uint8_t *row_mask, const float *weights, const uint8_t *dof_mask, const float *lower,
                const float *upper, const DwqParams *P, uint32_t *t, char *err, size_t errn, const char *who = "dwq_pack_table") {
    auto fail = [&](const char *msg, int idx) { snprintf(err, errn, "%s: %s (index %d)", who, msg, idx); return -1; };
    auto putf = [&](int k, float v) { memcpy(t + k, &v, 4); };
    if (!M || !Tg || !lower || !upper || !P || !t) return fail("a pointer is missing", 0);
    memset(t, 0, sizeof(uint32_t) * DWQ_TABLE_WORDS);
    uint32_t c[DWC_TABLE_WORDS];
    if (dwc::pack(M, Tg, c, err, errn, who) != 0) return -1;
    memcpy(t, c, sizeof(uint32_t) * DWQ_T_K);          // (dwl_pack_table's table begins with dwj_pack_table's)
    memcpy(t + DWQ_T_K, c + DWC_T_K, sizeof(uint32_t) * (1 + 4 * MAXK));
    const int m = 6 * Tg->count;
    uint32_t rows = 0;
    for (int r = 0; r < m; ++r) {
        if (!row_mask || row_mask[r]) rows |= 1u << r;
        if (weights && !(isfinite(weights[r]) && weights[r] > 0.0f)) return fail("a weight is not finite and positive", r);
        putf(DWQ_T_W + r, weights ? weights[r] : 1.0f);
    }
    if (rows == 0u) return fail("the row mask leaves no row active", 0);
    t[DWQ_T_ROWS] = rows;
    for (int j = 0; j < ND; ++j) {
        if (!dof_mask || dof_mask[j]) t[DWQ_T_DOFS + (j >> 5)] |= 1u << (j & 31);
        if (!(isfinite(lower[j]) && isfinite(upper[j]) && lower[j] <= upper[j])) return fail("a joint limit is not finite, or lower > upper", j);
        putf(DWQ_T_LIMIT + 2 * j, lower[j]);
        putf(DWQ_T_LIMIT + 2 * j + 1, upper[j]);
    }
    if (P->iterations < 1 || P->iterations > DWQ_MAX_ITERATIONS) return fail("iterations must be in 1..DWQ_MAX_ITERATIONS = 64", 0);
    if (!(P->damping >= DWQ_MIN_DAMPING && P->damping <= DWQ_MAX_DAMPING)) return fail("damping must be in [4e-3, 1e3]", 0);
    if (!(P->max_step > 0.0f)) return fail("max_step must be positive (+inf: no limit)", 0);
    if (!(isfinite(P->tol_pos) && P->tol_pos >= 0.0f && isfinite(P->tol_ang) && P->tol_ang >= 0.0f)) return fail("tol_pos and tol_ang must be finite and >= 0", 0);
    t[DWQ_T_PARAM] = (uint32_t)P->iterations;
    putf(DWQ_T_PARAM + 1, P->damping);
    putf(DWQ_T_PARAM + 2, P->max_step);
    putf(DWQ_T_PARAM + 3, P->tol_pos);
    putf(DWQ_T_PARAM + 4, P->tol_ang);
    t[DWQ_T_PARAM + 5] = (P->free_base ? DWQ_F_FREE_BASE : 0) | (P->clamp_limits ? DWQ_F_CLAMP : 0) | (P->targets_rel_root ? DWQ_F_REL_ROOT : 0);
    return 0;
}

}  // namespace dwq

#endif
