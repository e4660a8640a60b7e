/* dyros_stance_inverse_dynamics.h -- C-ABI of the stance inverse dynamics (isaacgymdyros_amd/csrc/dw_stance_inverse.hip; DESIGN.md section
 * 28): include/dyros_contact_inverse_dynamics.h's question -- which joint torques and contact wrenches give the robot a wanted acceleration
 *   M(q) a + h(q, nu) = [0_6; tau_joint] + J_c' f
 * -- asked per env for the contacts that env stands on, with the distance of every loaded contact from what a sole can deliver reported by
 * the same launch.  A batch of walking robots holds envs in double support, in left and in right single support and in flight at once:
 * `stance` [N, K] says which of the table's K contacts carry load in each env.  Opt-in and read-only: nothing here writes a buffer the step
 * reads.
 *
 * Coordinates, nu, p_ref, vel_at_com, mass_scale, dof_armature, contacts, rows, weights, f_ref, the sign of f and every input are
 * include/dyros_contact_inverse_dynamics.h's, word for word.  This header states what differs.
 *
 * The stance.  stance [N, K], uint8: a non-zero byte means that the contact carries load in that env (any non-zero byte is the same as 1);
 * NULL means that every contact does.  With A the env's active rows (the six rows of every active contact):
 *   r, J_c         as there: the same functions, the same bits, for all contacts
 *   G[i][j]        the sum over the rows r in A, ascending, of (J_b[r][i] / w_r) J_b[r][j]
 *   G = L D L', y  as there; y[k] = r[k] - s, s the sum over the rows in A ascending of J_b[r][k] f_ref[r]
 *   f[r]           r in A: f_ref[r] + (sum over k = 0 .. 5 ascending of J_b[r][k] y[k]) / w_r;  r not in A: +0.0, and f_ref[r] is not read
 *   tau_joint[j]   r[6 + j] - s, s the sum over the rows in A ascending of J_c[r][6 + j] f[r], visiting only the active contacts that have
 *                  joint j on their path
 *   contact_accel, tau_full   as there, for all rows: the stance does not enter
 * An inactive row is skipped, not multiplied by zero: a non-finite f_ref word of an inactive row leaves no trace.  So
 *   - an all-ones or NULL stance gives dwi_solve's bits in tau_joint, force, contact_accel and tau_full;
 *   - one active contact i with unit weights gives, in its six rows of force and in tau_joint, the bits of dwi_solve on the one-contact table
 *     of contact i, with f_ref that contact's six rows (or NULL): J_b is square then, and neither W nor f_ref matters.
 * An env with an EMPTY stance is in flight: nothing is factored, no word is NaN for finite inputs, force is +0.0, tau_joint is tau_full[6:]
 * and base_residual is tau_full[0:6], bit for bit: what the base would need and nothing delivers.
 *
 * The soles.  Every contact has a sole: a rectangle in the frame of the contact's moving body, centre c_s [3] and half extents h [2] along
 * the body's x and y, its normal the body's +z; and the table holds one friction coefficient mu.  Half extents of zero are a point, which
 * carries no moment.  Plane only, as include/dyros_sensors.h: the sole normal stands for the ground's.
 *
 * The margins.  For an active contact i on body b, with R_b the body's rotation (the chain walk's quaternion through dw_bodies.h's
 * quat_to_mat), pos the contact's point and (f, m) its wrench (rows 6 i .. 6 i + 2, and 6 i + 3 .. 6 i + 5), in float32, in this order, with
 * no division:
 *   f'[c]   = R_b[0][c] f[0] + R_b[1][c] f[1] + R_b[2][c] f[2]     (left to right), m'[c] alike from m: the wrench in the body frame
 *   d[c]    = c_s[c] - pos[c]
 *   m_s     = (m'[0] - (d[1] f'[2] - d[2] f'[1]),  m'[1] - (d[2] f'[0] - d[0] f'[2]),  m'[2] - (d[0] f'[1] - d[1] f'[0]))
 *   margins = (f'[2],  mu f'[2] - sqrt(f'[0] f'[0] + f'[1] f'[1]),  h[0] f'[2] - |m_s[1]|,  h[1] f'[2] - |m_s[0]|)
 * All four are >= 0 exactly when the sole can deliver the wrench: it pushes, it does not slide, and the centre of pressure lies inside the
 * rectangle.  An inactive contact's four words are +0.0.
 *   feasible       1 when the stance is not empty and every margin of every active contact is >= 0, else 0 (a NaN margin gives 0)
 *   base_residual  [k] = r[k] - s, s the sum over the rows in A ascending of J_b[r][k] f[r]: rounding when A is not empty
 *
 * Outputs, each optional (NULL skips it).  Every call writes every word of what it was given.
 *   tau_joint      [N, 33]    float32
 *   force          [N, m]     float32
 *   contact_accel  [N, m]     float32
 *   tau_full       [N, 39]    float32
 *   base_residual  [N, 6]     float32
 *   margins        [N, K, 4]  float32
 *   feasible       [N]        uint8
 * There is no regularisation, no pivoting and no non-finite guard: a non-finite input gives non-finite output for that env only.  The root
 * position never enters.
 *
 * The device table.  dwk_pack_table writes DWK_TABLE_WORDS 32-bit words.  Words [0, DWK_T_SOLE) are dwi_pack_table's DWI_TABLE_WORDS, bit
 * for bit (ones for the weights of a single contact included), then
 *   DWK_T_SOLE     [DWK_MAX_CONTACTS][5]   c_s [3] and h [2] as float bits (zeros past K)
 *   DWK_T_MU       [1]                     mu as float bits
 * and three words of padding, so that the table is a whole number of 16-byte pieces.
 */
#ifndef DYROS_STANCE_INVERSE_DYNAMICS_H
#define DYROS_STANCE_INVERSE_DYNAMICS_H

#include <stdint.h>

#include "dyros_contact_inverse_dynamics.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DWK_ABI_VERSION 1

#define DWK_NUM_BODIES    38    /* Gym rigid bodies */
#define DWK_NUM_DOF       33
#define DWK_NV            39    /* generalised velocities: 6 + DWK_NUM_DOF */
#define DWK_MAX_CONTACTS  4     /* = DWI_MAX_CONTACTS */
#define DWK_ROWS          6     /* constraint rows of a contact */
#define DWK_MAX_ROWS      24    /* = DWK_MAX_CONTACTS * DWK_ROWS */
#define DWK_SOLE_WORDS    5     /* a sole: centre [3], half extents [2] */
#define DWK_MARGINS       4     /* margins of a contact */
#define DWK_GROUP         4     /* envs per workgroup: DWI_GROUP */
#define DWK_LANES         64    /* lanes per env */

#define DWK_T_SOLE        1168  /* = DWI_TABLE_WORDS */
#define DWK_T_MU          1188
#define DWK_TABLE_WORDS   1192

int dwk_abi_version(void);
const char *dwk_last_error(void);
/* Host only, pure: validates everything dwi_pack_table validates, under this entry point's name, then the soles [count][DWK_SOLE_WORDS]
 * (NULL: every contact a point at its pos; else every word finite and no half extent negative) and mu (finite and positive), and writes
 * table_host [DWK_TABLE_WORDS].  0, or -1 with the last error set. */
int dwk_pack_table(const DwjModel *m, const DwcContacts *contacts, const float *weights, const float *soles, float mu, uint32_t *table_host);
/* One launch on `stream`.  The arguments are dwi_solve's, with table [DWK_TABLE_WORDS]; stance [N, K] uint8 is a device buffer or NULL
 * (every contact active); base_residual [N, 6], margins [N, K, 4] and feasible [N] (uint8) are further outputs, device buffers or NULL.  No
 * argument changes from call to call, nothing is allocated and nothing synchronises, so the call sits inside a captured rollout step.  0, or
 * -1 with the last error set; every refusal (num_envs < 1, a missing input, a table that is not 16-byte aligned, no output at all, a
 * non-finite gravity) happens before any launch. */
int dwk_solve(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
              const float *dof_armature, float gx, float gy, float gz, const float *accel, const float *force_ref, const uint8_t *stance,
              int32_t vel_at_com, float *tau_joint, float *force, float *contact_accel, float *tau_full, float *base_residual, float *margins,
              uint8_t *feasible, void *stream);

#ifdef __cplusplus
}
#endif

#endif
