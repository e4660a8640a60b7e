/* dyros_inverse_kinematics.h -- C-ABI of the inverse kinematics (isaacgymdyros_amd/csrc/dw_inverse_kinematics.hip):
 * the joint angles (and, when asked, the base pose) that put chosen bodies at wanted poses, by up to I damped-least-squares steps per env in
 * one launch.  Every other model tensor answers a question about the state the simulator is in; this one asks which state puts a foot or
 * a hand where the caller wants it.  Opt-in and read-only: nothing here writes a buffer the step reads.
 *
 * Coordinates and nu are include/dyros_jacobians.h's with vel_at_com = 0, word for word: base columns 0:3 move the base origin, columns 3:6
 * turn the base about its origin (world axes), column 6 + j is Gym DoF j.  Targets are include/dyros_contact_dynamics.h's contacts: a Gym
 * body (0..37) and a point pos [3] in its frame, K = 1 .. DWQ_MAX_TARGETS = 4 of them; a jointless body stands for the moving body it is
 * welded to; no two targets on one moving body.  Each target has six rows, world axes: the point's position, then the body's orientation;
 * m = 6 K.  A wanted pose is targets [N, K, 7]: the point's position, then the body's quaternion xyzw.
 *
 * The iteration.  Per env, with q = q0 (NULL: dof_state's positions) and the base pose of root_states, up to I times:
 *   1  the chain walk at (base, q): dwj's walk, velocities do not enter
 *   2  e_lin = (t_pos - base_pos) - (the point's offset from the base), the first difference formed first, so that a robot 640 m out loses
 *      nothing in the offset; with targets_rel_root the target already is that difference and the root position never enters
 *   3  e_ang = 2 sign(w) v of q_target (x) conj(q_body): the rotation vector of the error to first order, without a transcendental.  (The
 *      reference example's orientation_error returns sign(w) v, half of this; its controller's gain absorbs the factor.)  The target's
 *      quaternion is normalised on the way in; a norm outside [0.99, 1.01], or an error word that is not finite, makes this env's outputs
 *      NaN, its iters 0 and its converged 0 -- this env only
 *   4  done if every active position word has |e| <= tol_pos and every active orientation word |e| <= tol_ang: a done env takes no
 *      further update, its q is the iterate that passed
 *   5  J [m][39]: dwj's jac_word at the points; +0.0 in the columns outside the DoF mask, in columns 0:6 with a fixed base and in an
 *      inactive row (whose e is +0.0 too)
 *   6  A = J J' + lambda^2 W^-1: the lower triangle, A[i][j] = the sum over c = 0 .. 38 ascending of J[i][c] J[j][c], then on the
 *      diagonal + (lambda lambda) / w_i; mirrored.  An inactive row's diagonal is 1: the factor keeps its shape and every loop its bound
 *   7  A = L D L' right-looking without pivoting and the two sweeps, include/dyros_contact_dynamics.h's, on y = e; then dnu[c] = the sum
 *      over r = 0 .. m - 1 ascending of J[r][c] y[r]
 *   8  s = max_step / max_j |dnu[6 + j]| when that maximum exceeds max_step, else no scaling: dnu[c] = dnu[c] s for every c
 *   9  q[j] += dnu[6 + j] for the masked joints, then with clamp_limits q[j] = lower_j where q[j] < lower_j, upper_j where q[j] > upper_j;
 *      an unmasked joint is never touched.  With free_base x += dnu[0:3] and quat = normalise((dnu[3:6] / 2, 1) (x) quat)
 * and after the loop one more walk and the error rows at the returned q: `residual`, `err` and `converged` come from them.
 * A is symmetric positive definite for lambda > 0, so no pivoting is needed; dwq_pack_table takes lambda in [DWQ_MIN_DAMPING = 4e-3, 1e3]:
 * at 4e-3 the largest cond(A) over the 4096 seeded states with unit weights and a fixed base is 3.09e5 (both feet) and 6.20e5 (four
 * targets), inside the 8.0e5 that section 26 factors without pivoting (at 3e-3 four targets reach 1.1e6); at the default 0.05, the
 * reference's, it is 2.06e3 and 4.14e3.  A free base lowers it.  Float32, built with -ffp-contract=off; sinf / cosf
 * are the chain walk's only library calls.
 *
 * Outputs, each optional (NULL skips it).  Every call writes every word of what it was given.
 *   q          [N, 33] float32   the solved angles; an unmasked joint: q0's bits
 *   root_out   [N, 7]  float32   the base pose, position then quaternion xyzw: root_states' bits with a fixed base
 *   residual   [N, m]  float32   the error rows (not weighted) at the returned q; +0.0 on inactive rows
 *   err        [N, 2]  float32   the largest |residual| over the active position rows, over the active orientation rows (+0.0 with none)
 *   iters      [N]     int32     updates applied
 *   converged  [N]     uint8     1 where the returned q passes the test of step 4
 *
 * The device table.  dwq_pack_table validates the model as dwj_pack_table does and the targets as dwc_pack_table does its contacts, and
 * writes DWQ_TABLE_WORDS 32-bit words, which the caller uploads as an ordinary tensor.  Words [0, DWQ_T_K) are dwj_pack_table's, then
 *   DWQ_T_K       [1]                    K
 *   DWQ_T_TARGET  [DWQ_MAX_TARGETS][4]   the moving body, and pos as float bits (zeros past K)
 *   DWQ_T_ROWS    [1]                    the row mask, bit r for row r
 *   DWQ_T_W       [DWQ_MAX_ROWS]         the weights as float bits (zeros past m)
 *   DWQ_T_DOFS    [2]                    the DoF mask, bit j for Gym DoF j
 *   DWQ_T_LIMIT   [DWQ_NUM_DOF][2]       lower, upper as float bits
 *   DWQ_T_PARAM   [6]                    iterations, damping, max_step, tol_pos, tol_ang (float bits), flags (DWQ_F_*)
 * which is a whole number of 16-byte pieces.
 */
#ifndef DYROS_INVERSE_KINEMATICS_H
#define DYROS_INVERSE_KINEMATICS_H

#include <stdint.h>

#include "dyros_contact_dynamics.h"
#include "dyros_jacobians.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DWQ_ABI_VERSION 1

#define DWQ_NUM_BODIES      38    /* Gym rigid bodies */
#define DWQ_NUM_DOF         33
#define DWQ_NV              39    /* generalised velocities: 6 + DWQ_NUM_DOF */
#define DWQ_MAX_TARGETS     4     /* = DWC_MAX_CONTACTS */
#define DWQ_ROWS            6     /* rows of a target */
#define DWQ_MAX_ROWS        24    /* = DWQ_MAX_TARGETS * DWQ_ROWS */
#define DWQ_MAX_ITERATIONS  64
#define DWQ_GROUP           4     /* envs per workgroup */
#define DWQ_LANES           64    /* lanes per env */

#define DWQ_T_K             1124  /* = DWJ_TABLE_WORDS */
#define DWQ_T_TARGET        1125
#define DWQ_T_ROWS          1141
#define DWQ_T_W             1142
#define DWQ_T_DOFS          1166
#define DWQ_T_LIMIT         1168
#define DWQ_T_PARAM         1234
#define DWQ_TABLE_WORDS     1240

#define DWQ_F_FREE_BASE     1     /* flags of DWQ_T_PARAM + 5 */
#define DWQ_F_CLAMP         2
#define DWQ_F_REL_ROOT      4

#define DWQ_MIN_DAMPING     4e-3f
#define DWQ_MAX_DAMPING     1e3f

typedef struct DwqParams {
    int32_t iterations;                /* 1 .. DWQ_MAX_ITERATIONS */
    float damping;                     /* lambda, in [DWQ_MIN_DAMPING, DWQ_MAX_DAMPING] */
    float max_step;                    /* > 0, or +inf for none: the largest joint update of one iteration, rad */
    float tol_pos, tol_ang;            /* >= 0: m, rad */
    int32_t free_base;                 /* 0: columns 0:6 are held, the base stays; otherwise the base pose is solved for too */
    int32_t clamp_limits;              /* clamp the masked joints to [dof_lower, dof_upper] after every update */
    int32_t targets_rel_root;          /* the targets' positions are offsets from the base position */
} DwqParams;

int dwq_abi_version(void);
const char *dwq_last_error(void);
/* Host only, pure: validates the model as dwj_pack_table does, the targets as dwc_pack_table does its contacts (count in
 * 1..DWQ_MAX_TARGETS, every body id in 0..37, every pos finite, no two targets on one moving body), row_mask [6 count] (NULL: every row;
 * at least one row active), weights [6 count] (NULL: ones; each finite and positive), dof_mask [33] (NULL: every joint), dof_lower and
 * dof_upper [33] (finite, lower <= upper) and params, and writes table_host [DWQ_TABLE_WORDS].  0, or -1 with the last error set. */
int dwq_pack_table(const DwjModel *m, const DwcContacts *targets, const uint8_t *row_mask, const float *weights, const uint8_t *dof_mask,
                   const float *dof_lower, const float *dof_upper, const DwqParams *params, uint32_t *table_host);
/* One launch on `stream`.  table [DWQ_TABLE_WORDS], root_states [N,13], dof_state [N,33,2] and targets [N,K,7] are device buffers; q0
 * [N,33] is a device buffer or NULL (dof_state's positions); so are the outputs q [N,33], root_out [N,7], residual [N,m], err [N,2], iters
 * [N] int32 and converged [N] uint8.  K and m = 6 K come from the table.  No argument changes from call to call, nothing is allocated and
 * nothing synchronises, so the call sits inside a captured rollout step.  0, or -1 with the last error set; every refusal (num_envs < 1, a
 * missing input, a table that is not 16-byte aligned, no output at all) happens before any launch. */
int dwq_solve(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *q0, const float *targets,
              float *q, float *root_out, float *residual, float *err, int32_t *iters, uint8_t *converged, void *stream);

#ifdef __cplusplus
}
#endif

#endif
