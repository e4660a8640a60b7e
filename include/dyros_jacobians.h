/* dyros_jacobians.h -- C-ABI of the Jacobian and mass-matrix tensors (isaacgymdyros_amd/csrc/dw_jacobian.hip): what
 * acquire_jacobian_tensor / refresh_jacobian_tensors and acquire_mass_matrix_tensor / refresh_mass_matrix_tensors give at the Gym boundary,
 * computed from the bound root_states [N,13] and dof_state [N,33,2] by the chain of include/dyros_bodies.h.  Opt-in and read-only: nothing
 * here writes a buffer the step reads.
 *
 * Coordinates.  The generalised velocity is nu = [root_states[7:10], root_states[10:13], dof_vel[0:33]], DWJ_NV = 39 numbers, world axes:
 * the root row's own velocity words, whatever vel_at_com makes them mean, followed by dof_state[:, :, 1].  DoF j drives moving body j + 1.
 * p_ref is the point whose velocity the root row holds, as an offset from the base origin: 0, or R_0 c_0 (the base COM; c_0 = the inert_com
 * of Gym body 0's inertial record) when vel_at_com != 0.  x_b, R_b are moving body b's offset from the base and rotation (dyros_bodies.h),
 * a_j = R_{j+1} mv_axis[j+1] the world axis of DoF j.
 *
 * jacobian [N, K, 6, 39], float32, K = a list of Gym body ids (any order, repeats allowed).  Rows 0:3 linear, 3:6 angular, as in Gym; columns
 * 0:6 the root's linear then angular velocity, column 6 + j DoF j.  Defining identity: jacobian[e, r] nu[e] = words [7:13] of the same
 * body's row of dwb_refresh in the same vel_at_com mode.  So the point p of a row is the point whose velocity dwb_refresh reports: with
 * vel_at_com, x_m + R_m c_g for a Gym body g with an inertial record (m = its carrier), the carrier's origin x_m otherwise; the welded
 * bodies 7, 8, 15, 16 follow their carriers.  Then
 *   base block      [[I, -[p - p_ref]x], [0, I]]
 *   column 6 + j    [a_j x (p - x_{j+1}); a_j] when moving body j + 1 is the row's carrier or one of its ancestors
 *   anything else   +0.0 exactly (the diagonal of -[p - p_ref]x included)
 *   Gym body 0      [I 0; 0 I | 0] exactly
 *
 * mass_matrix [N, 39, 39], float32: the joint-space inertia in the same nu,
 *   M = sum_k w_k J_k,lin' J_k,lin + J_k,ang' (s_k R I_k R') J_k,ang over the DWJ_NUM_INERT inertial records,
 * J_k the Jacobian at the record's COM x_m + R_m c_k, s_k = mass_scale[e][inert_gym[k]] (1 when mass_scale is NULL), w_k = inert_mass[k] s_k,
 * I_k = inert_I[k] (xx, yy, zz, xy, xz, yz in the carrier's frame), R = R_m.  dof_armature[e][j] is added to entry [6 + j, 6 + j] when given.
 * It is computed as composite-rigid-body sums: for moving body i the mass, first moment and second moment ABOUT x_i (p_ref for the base) of
 * the records its subtree carries, F_i = that inertia applied to DoF i - 1's unit motion, and entry (i, j), j on the path from the base to i,
 * = the motion of j at x_i dotted with F_i.  Rows >= columns are formed and mirrored, so the output is symmetric bit for bit; entries that
 * couple joints on different branches are +0.0 exactly.  mass_matrix[:, 6:, 6:] is Gym's (num_dofs, num_dofs) matrix.
 *
 * com_jacobian [N, 3, 39] = mass_matrix[0:3, :] / sum_k w_k; com_jacobian nu = words [3:6] of dwb_refresh's com.
 *
 * The root position never enters: J and M of an env 640 m out are the bits of the same state at the origin.  There is no non-finite guard: a
 * non-finite input gives non-finite output for that env only.  Every call writes every word of its outputs, the structural zeros included.
 *
 * The device table.  dwj_pack_table validates a DwjModel on the host and writes DWJ_TABLE_WORDS 32-bit words, which the caller uploads as an
 * ordinary tensor.  Words [0, DWJ_T_ANC) are the table of dwb_pack_table (include/dyros_bodies.h) for the same model, then
 *   DWJ_T_ANC  [DWJ_NUM_MOVING][2]   bit b (of 64, low word first) set when moving body b >= 1 is body m or one of its ancestors
 *   DWJ_T_SUB  [DWJ_NUM_MOVING][2]   bit k set when inertial record k is carried by body i or one of its descendants
 *   DWJ_T_I    [DWJ_NUM_INERT][6]    inert_I
 */
#ifndef DYROS_JACOBIANS_H
#define DYROS_JACOBIANS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWJ_ABI_VERSION 1

#define DWJ_NUM_BODIES   38    /* Gym rigid bodies */
#define DWJ_NUM_MOVING   34    /* floating base + 33 hinge links */
#define DWJ_NUM_DOF      33
#define DWJ_NUM_INERT    36    /* inertial records */
#define DWJ_NV           39    /* generalised velocities: 6 + DWJ_NUM_DOF */
#define DWJ_JAC_ROWS     6
#define DWJ_GROUP        8     /* envs per workgroup, both kernels */
#define DWJ_LANES        32    /* lanes per env */

#define DWJ_T_ANC        772   /* = DWB_TABLE_WORDS */
#define DWJ_T_SUB        840
#define DWJ_T_I          908
#define DWJ_TABLE_WORDS  1124

typedef struct DwjModel {
    int32_t mv_parent[DWJ_NUM_MOVING];
    float mv_pos[DWJ_NUM_MOVING][3];
    float mv_rot0[DWJ_NUM_MOVING][9];
    float mv_axis[DWJ_NUM_MOVING][3];
    int32_t body_moving[DWJ_NUM_BODIES];
    int32_t inert_gym[DWJ_NUM_INERT];
    int32_t inert_mv[DWJ_NUM_INERT];
    float inert_mass[DWJ_NUM_INERT];
    float inert_com[DWJ_NUM_INERT][3];
    float inert_I[DWJ_NUM_INERT][6];
} DwjModel;

int dwj_abi_version(void);
const char *dwj_last_error(void);
/* Host only, pure: validates the model as dwb_pack_table does, and that inert_I is finite, and writes table_host [DWJ_TABLE_WORDS].  0, or -1
 * with the last error set. */
int dwj_pack_table(const DwjModel *m, uint32_t *table_host);
/* One launch on `stream`.  table [DWJ_TABLE_WORDS], root_states and dof_state are device buffers; body_ids_host is a HOST array of nb Gym body
 * ids, 1 <= nb <= 38, any order, repeats allowed, copied into the kernel's argument block (NULL: all 38 in order, nb 0 or 38).  jac
 * [N, nb, 6, 39].  No argument changes from call to call, nothing is allocated and nothing synchronises, so the call sits inside a captured
 * rollout step.  0, or -1 with the last error set; every refusal (num_envs < 1, a missing buffer, nb out of range, an id outside 0..37)
 * happens before any launch. */
int dwj_jacobian(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const int32_t *body_ids_host,
                 int32_t nb, int32_t vel_at_com, float *jac, void *stream);
/* One launch on `stream`.  mass_scale [N,38] and dof_armature [N,33] are device buffers or NULL; mm [N,39,39]; com_jac [N,3,39] or NULL.  The
 * same rules. */
int dwj_mass_matrix(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
                    const float *dof_armature, int32_t vel_at_com, float *mm, float *com_jac, void *stream);

#ifdef __cplusplus
}
#endif

#endif
