/* dyros_bodies.h -- C-ABI of the rigid-body state tensor (isaacgymdyros_amd/csrc/dw_bodies.hip): what
 * acquire_rigid_body_state_tensor / refresh_rigid_body_state_tensor give at the Gym boundary.  [N, 38, 13] = position, quaternion xyzw,
 * linear velocity and angular velocity of every Gym body in the world frame, computed from the bound root_states [N,13] and dof_state
 * [N,33,2] by the physics' own chain (oracle/dw_physics.c section 1), and optionally the centre of mass [N,7].  Opt-in and read-only:
 * nothing here writes a buffer the step reads.
 *
 * Moving bodies (the floating base and the 33 hinge links; moving body b > 0 is driven by DoF b - 1, p is its parent):
 *   base     x_0, v, w from the root row; q_0 = the root quaternion divided by its norm, as the physics does; R_0 = R(q_0)
 *   body b   x_b  = x_p + R_p mv_pos[b]
 *            q_b  = q_p * quat(mv_rot0[b]) * quat(mv_axis[b], angle_b),   R_b = R(q_b)     (= R_p mv_rot0[b] Rot(mv_axis[b], angle_b))
 *            w_b  = w_p + R_b mv_axis[b] rate_b
 *            vo_b = vo_p + w_p x (x_b - x_p)                                               (the velocity of the body ORIGIN)
 * Offsets from the base are accumulated on their own and the base position is added last, one rounding: a body's offset is as accurate
 * for an env whose origin lies 640 m out as for env 0.  Quaternions are multiplied down the chain from q_0: no matrix is turned into a
 * quaternion per env and no sign is canonicalised, so the sign follows the base's and does not flip from step to step.  (mv_rot0 is a
 * matrix in the model; dwb_pack_table turns it into a quaternion once, on the host, in double; its sign: w > 0, or for a half turn
 * the first of x, y, z that is not zero positive.)
 *
 * Gym body g is carried by moving body m = body_moving[g]; the four jointless foot bodies (Gym 7, 8, 15, 16) are welded to moving bodies 6
 * and 12 with a zero offset and no rotation, so a welded body's pose IS its carrier's.  Row g of the output:
 *   [0:3]   x_m
 *   [3:7]   q_m, xyzw
 *   [7:10]  vo_m + w_m x R_m c_g when vel_at_com != 0 and g has an inertial record (c_g = its inert_com, in the carrier's frame); vo_m otherwise
 *   [10:13] w_m
 * vel_at_com is the env's root_vel_at_com: with it set the root row's velocity is the base COM's, and vo_0 = root[7:10] - w x R_0 c_0, as the
 * physics undoes it.  Row 0 is the 13 words of the root row bit for bit, in either mode.
 *
 * com [N,7]: words 0..2 = sum_k w_k (x_m + R_m c_k) / sum_k w_k over the DWB_NUM_INERT inertial records (formed as an offset from the base,
 * the base added last), 3..5 = the same average of the records' COM velocities vo_m + w_m x R_m c_k, 6 = sum_k w_k;
 * w_k = inert_mass[k] * mass_scale[e][inert_gym[k]], the scale 1 when mass_scale is NULL.
 *
 * There is no non-finite guard: a non-finite input gives non-finite rows for that env only.
 *
 * The device table.  dwb_pack_table validates a DwbModel on the host and writes DWB_TABLE_WORDS 32-bit words (integers, or the bits of
 * floats), which the caller uploads as an ordinary tensor; the library neither allocates nor copies from host memory.  Layout:
 *   DWB_T_NLEAF              number of leaves of the kinematic tree (<= DWB_MAX_LEAVES)
 *   DWB_T_PATHLEN [DWB_MAX_LEAVES]              bodies on the path from the base's children down to leaf l
 *   DWB_T_PATH    [DWB_MAX_LEAVES][DWB_MAX_DEPTH] the path's moving bodies, base side first; bit 8 (DWB_PATH_OWNER) set where this path is the
 *                                            first to hold the body (that lane stores the body's state)
 *   DWB_T_MV      [DWB_NUM_MOVING][DWB_MV_WORDS]   parent, mv_pos[3], quat(mv_rot0) xyzw, mv_axis[3]
 *   DWB_T_CARRIER [DWB_NUM_BODIES]           body_moving
 *   DWB_T_RECORD  [DWB_NUM_BODIES]           the Gym body's inertial record, or -1
 *   DWB_T_INERT   [DWB_NUM_INERT][DWB_INERT_WORDS] inert_gym, inert_mv, inert_mass, inert_com[3]
 */
#ifndef DYROS_BODIES_H
#define DYROS_BODIES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWB_ABI_VERSION 1

#define DWB_NUM_BODIES   38    /* Gym rigid bodies */
#define DWB_NUM_MOVING   34    /* floating base + 33 hinge links */
#define DWB_NUM_DOF      33
#define DWB_NUM_INERT    36    /* inertial records */
#define DWB_ROW          13    /* words of a body's row */
#define DWB_COM_WORDS    7
#define DWB_GROUP        16    /* envs per workgroup */
#define DWB_LANES        16    /* lanes per env */
#define DWB_MAX_LEAVES   8     /* root-to-leaf paths of the tree: a lane each */
#define DWB_MAX_DEPTH    12    /* bodies on a path below the base */
#define DWB_PATH_OWNER   256

#define DWB_MV_WORDS     11
#define DWB_INERT_WORDS  6
#define DWB_T_NLEAF      0
#define DWB_T_PATHLEN    1
#define DWB_T_PATH       9
#define DWB_T_MV         105
#define DWB_T_CARRIER    479
#define DWB_T_RECORD     517
#define DWB_T_INERT      555
#define DWB_TABLE_WORDS  772   /* 771 used, padded to 16 bytes */

typedef struct DwbModel {
    int32_t mv_parent[DWB_NUM_MOVING];
    float mv_pos[DWB_NUM_MOVING][3];
    float mv_rot0[DWB_NUM_MOVING][9];
    float mv_axis[DWB_NUM_MOVING][3];
    int32_t body_moving[DWB_NUM_BODIES];
    int32_t inert_gym[DWB_NUM_INERT];
    int32_t inert_mv[DWB_NUM_INERT];
    float inert_mass[DWB_NUM_INERT];
    float inert_com[DWB_NUM_INERT][3];
} DwbModel;

int dwb_abi_version(void);
const char *dwb_last_error(void);
/* Host only, pure: validates the model (parents precede children, every index in range, every Gym body has exactly one carrier and at most
 * one inertial record, at most DWB_MAX_LEAVES leaves no deeper than DWB_MAX_DEPTH) and writes table_host [DWB_TABLE_WORDS].  0, or -1 with
 * dwb_last_error() set. */
int dwb_pack_table(const DwbModel *m, uint32_t *table_host);
/* One launch on `stream`.  table [DWB_TABLE_WORDS], root_states, dof_state and mass_scale [N,38] (or NULL) are device buffers; body_ids_host
 * is a HOST array of nb Gym body ids, 1 <= nb <= 38, any order, repeats allowed, copied into the kernel's argument block (NULL: all 38 in
 * order, nb 0 or 38).  states [N, nb, 13] or NULL, com [N,7] or NULL, at least one given.  No argument changes from call to call, nothing
 * is allocated and nothing synchronises, so the call sits inside a captured rollout step.  0, or -1 with dwb_last_error() set; every
 * refusal (num_envs < 1, a missing buffer, nb out of range, an id outside 0..37) happens before any launch. */
int dwb_refresh(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
                const int32_t *body_ids_host, int32_t nb, int32_t vel_at_com, float *states, float *com, void *stream);

#ifdef __cplusplus
}
#endif

#endif
