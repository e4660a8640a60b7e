/* dyros_contact_dynamics.h -- C-ABI of the contact-consistent dynamics (isaacgymdyros_amd/csrc/dw_contact_dynamics.hip; DESIGN.md section
 * 26): the equation of motion under rigid contact constraints,
 *   M(q) nu_dot + h(q, nu) = b + J_c' f,    J_c nu_dot + Jd_c nu = gamma,
 * solved for nu_dot and f in one launch from the bound root_states [N,13] and dof_state [N,33,2].  Opt-in and read-only: nothing here
 * writes a buffer the step reads.
 *
 * Coordinates, nu, p_ref, vel_at_com, mass_scale and dof_armature are include/dyros_jacobians.h's, word for word: nu = [root_states[7:10],
 * root_states[10:13], dof_vel[0:33]], DWC_NV = 39 numbers, world axes; DoF j is word 6 + j and drives moving body j + 1; M is
 * dwj_mass_matrix's matrix, formed and factored by the arithmetic of dwl_solve (include/dyros_forward_dynamics.h): the same bits.
 *
 * Contacts.  A contact is a Gym body (0..37) and a point pos [3] in that body's frame.  A jointless body (Gym 7, 8, 15, 16) stands for the
 * moving body it is welded to, with no offset and no rotation.  There are K contacts, 1 .. DWC_MAX_CONTACTS = 4.  Each contributes six
 * constraint rows in world axes: the point's linear velocity, then the body's angular velocity, so m = 6 K <= 24.  Two contacts carried by
 * the same moving body are refused when the table is packed: a rigid body has six freedoms, so the second contact's rows would be dependent.
 *
 * The system.  b = rhs - sub as in dwl_solve: rhs = [0_6; tau_joint] + other generalised forces, sub the slot for the bias h
 * (dwn_inverse_dynamics).  f [m] is the wrench the environment applies to the robot at each contact point: force, then moment about the
 * point, in world axes.  gamma [m] is the contact frames' commanded acceleration; NULL means zero, so the feet stay put.
 *
 * The solve.  Y = M^-1 J_c' (dwl_solve's sweeps over dwl_solve's factor), A = J_c Y, x0 = M^-1 b, A f = (gamma - Jd_c nu) - J_c x0,
 * nu_dot = x0 + Y f.  The right side is evaluated in the order written: 0 - a is exact, so a NULL gamma and a gamma of zeros give the same
 * bits.  A is symmetric positive definite; it is factored densely as L D L' without pivoting.  There is no regularisation and no non-finite
 * guard: a singular A, or a non-finite input, gives non-finite output for that env only.
 *
 * Outputs, float32, each optional (NULL skips it).  Every call writes every word of what it was given.
 *   jc          [N, m, 39]  J_c.  Row 6 i + c of contact i at P = x_b + R_b pos (b its moving body): linear rows [I, -[P - p_ref]x] on the base
 *                           columns and a_j x (P - x_j) on joint j; angular rows [0, I | a_j].  A joint off the path from the base to the
 *                           carrying body is +0.0 exactly; the identity blocks are 1.0 and +0.0 exactly.
 *   jdnu        [N, m]      Jd_c nu: the point's classical acceleration xdd_b + alpha_b x r + omega_b x (omega_b x r), r = R_b pos, and the
 *                           body's angular acceleration alpha_b, both at nu_dot = 0 (the recursion of include/dyros_dynamics.h)
 *   minv_jt     [N, m, 39]  row r is M^-1 jc[r]: the bits of dwl_solve's x with rhs = jc[r]
 *   lambda_inv  [N, m, m]   A = J_c M^-1 J_c'; rows >= columns are taken and mirrored, so the output is symmetric bit for bit
 *   lambda      [N, m, m]   the contact-space inertia A^-1, as solves of the identity's columns, mirrored the same way
 *   accel       [N, R, 39]  nu_dot for rhs [N, R, 39], R in 1 .. DWC_MAX_RHS = 8, sub [N, 39] or NULL, gamma [N, m] or NULL
 *   force       [N, R, m]   f
 * Every right-hand side is solved on its own: the bits of accel[e, r] and force[e, r] do not depend on R or on the other right-hand sides.
 * The dynamically consistent inverse lambda @ minv_jt and the contact null-space projector I - minv_jt' lambda jc are one bmm each of these.
 * The root position never enters: an env 640 m out gets the bits of the same state at the origin.
 *
 * The device table.  dwc_pack_table validates a DwjModel as dwl_pack_table does, and the contacts, and writes DWC_TABLE_WORDS 32-bit words,
 * which the caller uploads as an ordinary tensor.  Words [0, DWC_T_K) are the table of dwl_pack_table for the same model, then
 *   DWC_T_K        [1]                     K
 *   DWC_T_CONTACT  [DWC_MAX_CONTACTS][4]   the moving body, and pos as float bits (zeros past K)
 * and three words of padding, so that the table is a whole number of 16-byte pieces.
 */
#ifndef DYROS_CONTACT_DYNAMICS_H
#define DYROS_CONTACT_DYNAMICS_H

#include <stdint.h>

#include "dyros_forward_dynamics.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DWC_ABI_VERSION 1

#define DWC_NUM_BODIES    38    /* Gym rigid bodies */
#define DWC_NUM_DOF       33
#define DWC_NV            39    /* generalised velocities: 6 + DWC_NUM_DOF */
#define DWC_MAX_CONTACTS  4
#define DWC_ROWS          6     /* constraint rows of a contact */
#define DWC_MAX_ROWS      24    /* = DWC_MAX_CONTACTS * DWC_ROWS: the column batch of dwl_solve */
#define DWC_MAX_RHS       8     /* right-hand sides of one call at the most */
#define DWC_GROUP         3     /* envs per workgroup */
#define DWC_LANES         64    /* lanes per env */

#define DWC_T_K           1960  /* = DWL_TABLE_WORDS */
#define DWC_T_CONTACT     1961
#define DWC_TABLE_WORDS   1980

typedef struct DwcContacts {
    int32_t count;
    int32_t body[DWC_MAX_CONTACTS];          /* Gym body ids */
    float pos[DWC_MAX_CONTACTS][3];          /* in the body's frame */
} DwcContacts;

int dwc_abi_version(void);
const char *dwc_last_error(void);
/* Host only, pure: validates the model as dwl_pack_table does and the contacts (count in 1..DWC_MAX_CONTACTS, every body id in 0..37, every
 * pos finite, no two contacts on one moving body), and writes table_host [DWC_TABLE_WORDS].  0, or -1 with the last error set. */
int dwc_pack_table(const DwjModel *m, const DwcContacts *contacts, uint32_t *table_host);
/* One launch on `stream`.  table [DWC_TABLE_WORDS], root_states [N,13] and dof_state [N,33,2] are device buffers; mass_scale [N,38],
 * dof_armature [N,33], rhs [N,nrhs,39], sub [N,39] and gamma [N,m] are device buffers or NULL; so are the outputs.  m = 6 K comes from the
 * table.  No argument changes from call to call, nothing is allocated and nothing synchronises, so the call sits inside a captured rollout
 * step.  0, or -1 with the last error set; every refusal (num_envs < 1, a missing input, a table that is not 16-byte aligned, rhs without
 * accel or force, accel or force without rhs, sub or gamma without rhs, nrhs outside 1..DWC_MAX_RHS when rhs is given, no output at all)
 * happens before any launch.  nrhs is not read when rhs is NULL. */
int dwc_solve(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
              const float *dof_armature, int32_t vel_at_com, const float *rhs, int32_t nrhs, const float *sub, const float *gamma, float *jc,
              float *jdnu, float *minv_jt, float *lambda_inv, float *lambda, float *accel, float *force, void *stream);

#ifdef __cplusplus
}
#endif

#endif
