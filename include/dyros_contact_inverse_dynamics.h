/* dyros_contact_inverse_dynamics.h -- C-ABI of the contact inverse dynamics (isaacgymdyros_amd/csrc/dw_contact_inverse.hip; DESIGN.md
 * section 27): the joint torques and the contact wrenches that give a floating-base robot a wanted acceleration while its contacts carry
 * the base,
 *   M(q) a + h(q, nu) = [0_6; tau_joint] + J_c' f,
 * solved for tau_joint [33] and f [m] in one launch from the bound root_states [N,13] and dof_state [N,33,2] and the caller's a = nu_dot
 * [N,39].  It is the inverse of dwc_solve (include/dyros_contact_dynamics.h), which answers: this torque, these contacts, which
 * acceleration and which ground reaction.  Opt-in and read-only: nothing here writes a buffer the step reads.
 *
 * Coordinates, nu, p_ref, vel_at_com, mass_scale and dof_armature are include/dyros_jacobians.h's, word for word.  Contacts are
 * include/dyros_contact_dynamics.h's: a Gym body (0..37) and a point pos [3] in its frame, K = 1 .. DWI_MAX_CONTACTS = 4 of them, six rows
 * each (the point's linear velocity, the body's angular velocity, world axes), m = 6 K; a jointless body stands for the moving body it is
 * welded to; no two contacts on one moving body.  f has that header's sign: the wrench the environment applies to the robot at the point
 * (force, then moment about the point, world axes).
 *
 * The equation.  For the caller's a [39] (NULL: zero):
 *   r             = tau(a)                       dwn_inverse_dynamics's M a + h, all 39 rows (dof_armature on the joints when given)
 *   J_c           = [J_b | J_j]                  m x 6 base columns, m x 33 joint columns
 *   f             = f_ref + W^-1 J_b y,   G y = r[0:6] - J_b' f_ref,   G = J_b' W^-1 J_b   (6 x 6, symmetric positive definite)
 *   tau_joint     = r[6:] - J_j' f
 *   contact_accel = J_c a + Jd_c nu              the points' classical acceleration and the bodies' alpha under (q, nu, a)
 * f is the wrench set closest to f_ref in the W norm (W = diag(weights), m positive numbers) that carries the base rows exactly:
 * J_b' f = r[0:6].  With one contact J_b is square, f is unique, and neither W nor f_ref matters: dwi_pack_table then writes ones for the
 * weights, so the bits do not depend on them.  With two or more, the weights say how dear moments are against forces, and one contact
 * against another; f_ref (NULL: zero) is a prior such as "all weight on the stance foot".
 *
 * Round trip.  (a, f) is the unique solution of dwc_solve's system for b = [0; tau_joint] - h and gamma = contact_accel.
 *
 * Feasibility is not decided here: whether the contacts can deliver f (unilateral, friction, centre of pressure inside the sole) is for the
 * caller to read from `force`.  There is no regularisation, no pivoting and no non-finite guard: a non-finite input gives non-finite output
 * for that env only.  cond(G) stays below 7 with unit weights and below 40 with moments weighted 10 x.
 *
 * The arithmetic, in float32, in this order:
 *   r              the chain walk, records and subtree sums of dwn_inverse_dynamics with a: the same functions, the same bits
 *   J_c[r][c]      dwj's jac_word at the contact's point: the bits of dwc_solve's jc
 *   G[i][j]        i >= j, 21 words: the sum over the rows r = 0 .. m - 1, ascending, of (J_b[r][i] / w_r) J_b[r][j]; mirrored
 *   G = L D L'     right-looking, no pivoting: column j = 0 .. 4, G[i][k] -= (G[i][j] / G[j][j]) G[k][j] for j < k <= i; then L[i][j] =
 *                  G[i][j] / G[j][j]
 *   y              y[k] = r[k] - s, s the sum over the rows ascending of J_b[r][k] f_ref[r] (f_ref NULL: zeros, the same bits); then the
 *                  forward sweep (columns ascending), the division by D and the backward sweep (rows descending)
 *   f[r]           f_ref[r] + (sum over k = 0 .. 5 ascending of J_b[r][k] y[k]) / w_r
 *   tau_joint[j]   r[6 + j] - s, s the sum over the rows ascending of J_c[r][6 + j] f[r], visiting only the contacts that have joint j on the
 *                  path from the base to their body (the others' words are +0.0 in J_c)
 *   contact_accel  row 6 i + c: xdd_b + alpha_b x d + omega_b x (omega_b x d), d = R_b pos; row 6 i + 3 + c: alpha_b; the chain walk's words
 *                  taken WITH a (dwc_solve's jdnu is the same formula at nu_dot = 0)
 *
 * Outputs, float32, each optional (NULL skips it).  Every call writes every word of what it was given.
 *   tau_joint      [N, 33]
 *   force          [N, m]
 *   contact_accel  [N, m]
 *   tau_full       [N, 39]   r: the bits of dwn_inverse_dynamics's tau for the same inputs (a NULL: its tau for zeros, a zero's sign apart)
 * The root position never enters: an env 640 m out gets the bits of the same state at the origin.
 *
 * The device table.  dwi_pack_table validates the model as dwn_pack_table does and the contacts as dwc_pack_table does, and the weights, and
 * writes DWI_TABLE_WORDS 32-bit words, which the caller uploads as an ordinary tensor.  Words [0, DWI_T_K) are dwn_pack_table's, then
 *   DWI_T_K        [1]                     K
 *   DWI_T_CONTACT  [DWI_MAX_CONTACTS][4]   the moving body, and pos as float bits (zeros past K): dwc_pack_table's words
 *   DWI_T_W        [DWI_MAX_ROWS]          the weights as float bits (ones for K = 1; zeros past m)
 * and three words of padding, so that the table is a whole number of 16-byte pieces.
 */
#ifndef DYROS_CONTACT_INVERSE_DYNAMICS_H
#define DYROS_CONTACT_INVERSE_DYNAMICS_H

#include <stdint.h>

#include "dyros_contact_dynamics.h"
#include "dyros_dynamics.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DWI_ABI_VERSION 1

#define DWI_NUM_BODIES    38    /* Gym rigid bodies */
#define DWI_NUM_DOF       33
#define DWI_NV            39    /* generalised velocities: 6 + DWI_NUM_DOF */
#define DWI_MAX_CONTACTS  4     /* = DWC_MAX_CONTACTS */
#define DWI_ROWS          6     /* constraint rows of a contact */
#define DWI_MAX_ROWS      24    /* = DWI_MAX_CONTACTS * DWI_ROWS */
#define DWI_GROUP         4     /* envs per workgroup: DWN_GROUP */
#define DWI_LANES         64    /* lanes per env */

#define DWI_T_K           1124  /* = DWN_TABLE_WORDS */
#define DWI_T_CONTACT     1125
#define DWI_T_W           1141
#define DWI_TABLE_WORDS   1168

int dwi_abi_version(void);
const char *dwi_last_error(void);
/* Host only, pure: validates the model as dwn_pack_table does, the contacts as dwc_pack_table does (count in 1..DWI_MAX_CONTACTS, every body
 * id in 0..37, every pos finite, no two contacts on one moving body) and the weights [6 count] (NULL: ones; each finite and positive), and
 * writes table_host [DWI_TABLE_WORDS].  0, or -1 with the last error set. */
int dwi_pack_table(const DwjModel *m, const DwcContacts *contacts, const float *weights, uint32_t *table_host);
/* One launch on `stream`.  table [DWI_TABLE_WORDS], root_states [N,13] and dof_state [N,33,2] are device buffers; mass_scale [N,38],
 * dof_armature [N,33], accel [N,39] and force_ref [N,m] are device buffers or NULL; (gx, gy, gz) is the gravity vector; so are the outputs
 * tau_joint [N,33], force [N,m], contact_accel [N,m] and tau_full [N,39].  m = 6 K comes from the table.  No argument changes from call to
 * call, nothing is allocated and nothing synchronises, so the call sits inside a captured rollout step.  0, or -1 with the last error set;
 * every refusal (num_envs < 1, a missing input, a table that is not 16-byte aligned, no output at all, a non-finite gravity) happens before
 * any launch. */
int dwi_solve(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
              const float *dof_armature, float gx, float gy, float gz, const float *accel, const float *force_ref, int32_t vel_at_com,
              float *tau_joint, float *force, float *contact_accel, float *tau_full, void *stream);

#ifdef __cplusplus
}
#endif

#endif
