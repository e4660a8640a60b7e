/* dyros_forward_dynamics.h -- C-ABI of the forward dynamics (isaacgymdyros_amd/csrc/dw_forward_dynamics.hip): the
 * equation of motion
 *   M(q) nu_dot + h(q, nu) = [0_6; tau_joint] + sum J' f_ext
 * solved for nu_dot.  One launch forms the joint-space inertia M of include/dyros_jacobians.h from the bound root_states [N,13] and dof_state
 * [N,33,2], factors it as M = L' D L on the sparsity pattern of the kinematic tree, and gives the solutions of M x = rhs - sub, the factor
 * and the inverse.  Opt-in and read-only: nothing here writes a buffer the step reads.
 *
 * Coordinates (dyros_jacobians.h's, word for word).  nu = [root_states[7:10], root_states[10:13], dof_vel[0:33]], DWL_NV = 39 numbers, world
 * axes.  p_ref is the point whose velocity the root row holds, as an offset from the base origin: 0, or R_0 c_0 (the base COM) when
 * vel_at_com != 0.  DoF j is word 6 + j and drives moving body j + 1.  M is dwj_mass_matrix's matrix for the same root_states, dof_state,
 * mass_scale, dof_armature and vel_at_com, formed by the same arithmetic: the same bits.  mass_scale NULL: nominal masses; dof_armature NULL:
 * no armature on the joints' diagonal.
 *
 * The factorisation.  Bodies are numbered parents first, so M = L' D L with L unit lower triangular and D diagonal (Featherstone's LTDL: rows
 * 38 down to 0 are eliminated, row k's multipliers a = M[k][i] / M[k][k] taken from what the rows above k have left of it) has no fill-in: a
 * row of L can be non-zero only where the same row of M can.  The pattern of the lower triangle, diagonal included, is
 *   rows 0..5      every column up to the diagonal (the base block is dense: M[0:3, 0:3] is diagonal and fills in)
 *   row 6 + j      columns 0..5, column 6 + i for every joint i that moves an ancestor of body j + 1 (ascending), column 6 + j
 * DWL_PATTERN = 396 of the 780 entries, at most DWL_MAX_ROW = 17 in a row.  It is derived from mv_parent on the host, never from numerical
 * zeros.  An env's store holds those 396 words, row after row.
 *
 * Outputs, float32, each optional (NULL skips it):
 *   x       [N, nrhs, 39]  x[e, r] = M^-1 (rhs[e, r] - sub[e]), rhs [N, nrhs, 39], sub [N, 39] or NULL (the slot of dwn_inverse_dynamics' bias h:
 *                          with rhs = [0_6; tau_joint] + sum J' f_ext and sub = h, x is nu_dot).  rhs - 0 is exact, so sub NULL and a sub of zeros
 *                          give the same bits.  Every right-hand side is solved on its own: the bits of x[e, r] do not depend on nrhs or on the
 *                          other right-hand sides.  The solve runs L'^-1 (rows 38 down to 1), D^-1 (a division) and L^-1 (columns 0 up to 37, so that a
 *                          word's products are subtracted in ascending column order) over the pattern.
 *   factor  [N, 39, 39]    D on the diagonal, L strictly below it (its unit diagonal is implied), +0.0 above the diagonal and at every entry
 *                          outside the pattern.
 *   minv    [N, 39, 39]    M^-1: column c is the solve of the identity's column c; rows >= columns are taken and mirrored, so the output is
 *                          symmetric bit for bit, as M is.  The base is free: minv[:, 6:, 6:] is NOT the inverse of mass_matrix[:, 6:, 6:].
 *
 * The root position never enters: an env 640 m out gets the bits of the same state at the origin.  There is no non-finite guard: a
 * non-finite input gives non-finite output for that env only.  Every call writes every word of the outputs it was given.  M is symmetric
 * positive definite for every state of the chain, so there is no pivoting; its condition number is 3 to 4 10^4 with the task's armatures.
 *
 * The device table.  dwl_pack_table validates a DwjModel as dwj_pack_table does and writes DWL_TABLE_WORDS 32-bit words, which the caller
 * uploads as an ordinary tensor.  Words [0, DWL_T_ROW) are the table of dwj_pack_table (include/dyros_jacobians.h) for the same model, then
 *   DWL_T_ROW  [DWL_NV + 1]     the first pattern word of every row, and DWL_PATTERN
 *   DWL_T_COL  [DWL_PATTERN]    row << 8 | column of every pattern word
 *   DWL_T_TROW [DWL_NV + 1]     the pattern by columns: the first word in DWL_T_TCOL of every column, and DWL_PATTERN - DWL_NV
 *   DWL_T_TCOL [DWL_PATTERN - DWL_NV]  row << 16 | pattern word of every word below the diagonal, column after column, rows ascending
 * and three words of padding, so that the table is a whole number of 16-byte pieces.
 */
#ifndef DYROS_FORWARD_DYNAMICS_H
#define DYROS_FORWARD_DYNAMICS_H

#include <stdint.h>

#include "dyros_jacobians.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DWL_ABI_VERSION 1

#define DWL_NUM_BODIES   38    /* Gym rigid bodies */
#define DWL_NUM_MOVING   34    /* floating base + 33 hinge links */
#define DWL_NUM_DOF      33
#define DWL_NV           39    /* generalised velocities: 6 + DWL_NUM_DOF */
#define DWL_PATTERN      396   /* words of the lower triangle of L and D that can be non-zero */
#define DWL_MAX_ROW      17    /* pattern words of a row at the most: 6 base columns, 10 ancestors, the diagonal */
#define DWL_MAX_RHS      8     /* right-hand sides of one call at the most */
#define DWL_GROUP        4     /* envs per workgroup */
#define DWL_LANES        64    /* lanes per env */

#define DWL_T_ROW        1124  /* = DWJ_TABLE_WORDS */
#define DWL_T_COL        1164
#define DWL_T_TROW       1560
#define DWL_T_TCOL       1600
#define DWL_TABLE_WORDS  1960

int dwl_abi_version(void);
const char *dwl_last_error(void);
/* Host only, pure: validates the model as dwj_pack_table does, and that no row of the pattern holds more than DWL_MAX_ROW words, and writes
 * table_host [DWL_TABLE_WORDS].  0, or -1 with the last error set. */
int dwl_pack_table(const DwjModel *m, uint32_t *table_host);
/* One launch on `stream`.  table [DWL_TABLE_WORDS], root_states [N,13] and dof_state [N,33,2] are device buffers; mass_scale [N,38],
 * dof_armature [N,33], rhs [N,nrhs,39] and sub [N,39] are device buffers or NULL.  x [N,nrhs,39], factor [N,39,39] and minv [N,39,39] are
 * device buffers or NULL.  No argument changes from call to call, nothing is allocated and nothing synchronises, so the call sits inside a
 * captured rollout step.  0, or -1 with the last error set; every refusal (num_envs < 1, a missing input, a table that is not 16-byte
 * aligned, rhs without x, x without rhs, sub without rhs, nrhs outside 1..DWL_MAX_RHS when rhs is given, no output at all) happens before
 * any launch.  nrhs is not read when rhs is NULL. */
int dwl_solve(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
              const float *dof_armature, int32_t vel_at_com, const float *rhs, int32_t nrhs, const float *sub, float *x, float *factor,
              float *minv, void *stream);

#ifdef __cplusplus
}
#endif

#endif
