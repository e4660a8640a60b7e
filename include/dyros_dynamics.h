/* dyros_dynamics.h -- C-ABI of the bias-force, gravity, inverse-dynamics and momentum tensors (isaacgymdyros_amd/csrc/dw_dynamics.hip;
 * DESIGN.md section 24): the right-hand half of the equation of motion
 *   M(q) nu_dot + h(q, nu) = [0_6; tau_joint] + sum J' f_ext
 * in the coordinates of include/dyros_jacobians.h, computed from the bound root_states [N,13] and dof_state [N,33,2] by one recursive
 * Newton-Euler pass over the chain of include/dyros_bodies.h.  Opt-in and read-only: nothing here writes a buffer the step reads.
 *
 * Coordinates (dyros_jacobians.h's, word for word).  nu = [root_states[7:10], root_states[10:13], dof_vel[0:33]], DWN_NV = 39 numbers, world
 * axes.  p_ref is the point whose velocity the root row holds, as an offset from the base origin: 0, or R_0 c_0 (the base COM) when
 * vel_at_com != 0.  x_b, R_b are moving body b's offset from the base and rotation, a_j = R_{j+1} mv_axis[j+1] the world axis of DoF j.
 * nu_dot = a is the component-wise time derivative of nu: a[0:3] the classical acceleration of the material point p_ref, a[3:6] the base's
 * angular acceleration in world axes, a[6:] the joint accelerations.
 *
 * Definition, over the DWN_NUM_INERT inertial records; record k has carrier m:
 *   f_k = w_k (cdd_k - g)                      w_k = inert_mass[k] mass_scale[e][inert_gym[k]]   (mass_scale NULL: 1)
 *   n_k = Ib_k alpha_m + omega_m x (Ib_k omega_m)   Ib_k = s_k R_m I_k R_m'
 *   tau(a) = sum_k J_k,lin' f_k + J_k,ang' n_k   (+ dof_armature[e][j] a[6 + j] on the joints, when given)
 * J_k = dyros_jacobians.h's Jacobian at the record's COM; g = the gravity vector (gx, gy, gz); cdd_k, omega_m, alpha_m the classical COM
 * acceleration, angular velocity and angular acceleration that (q, nu, a) imply:
 *   base    omega_0 = nu[3:6], alpha_0 = a[3:6], xdd_0 = a[0:3] - alpha_0 x p_ref - omega_0 x (omega_0 x p_ref)
 *   child b of p (DoF j = b - 1)   omega_b = omega_p + a_j qd_j
 *                                  alpha_b = alpha_p + a_j qdd_j + omega_p x a_j qd_j
 *                                  xdd_b = xdd_p + alpha_p x r + omega_p x (omega_p x r),  r = x_b - x_p
 *   record  cdd_k = xdd_m + alpha_m x d + omega_m x (omega_m x d),  d = R_m c_k
 * These are Kane's equations with dyros_jacobians.h's partial velocities, so they hold for these quasi-velocities without further terms.
 *
 * Outputs, float32, each optional (NULL skips it):
 *   bias     [N, 39]  h(q, nu) = tau(0): Coriolis, centrifugal and gravity forces.  It holds NO joint damping, NO friction and NO actuator
 *                     term: those belong to the step's joint model, not to the rigid-body equation.
 *   gravity  [N, 39]  G(q) = tau(0) at nu = 0 = -sum_k J_k,lin' w_k g.  gravity[:, 6:] is the gravity-compensation torque;
 *                     gravity[:, 0:3] = -g sum_k w_k.
 *   tau      [N, 39]  tau(a) = M a + h for the caller's accel [N, 39]; the armature on the joints' diagonal as for dwj_mass_matrix, when given.
 *   momentum [N, 6]   linear momentum sum_k w_k cd_k, then the angular momentum ABOUT THE CENTRE OF MASS, world axes.
 * bias[:, 0:3] - gravity[:, 0:3] is the rate of change of linear momentum that the velocities alone cause.
 *
 * It is computed as subtree sums: for moving body i the force and the moment ABOUT x_i (p_ref for the base) of the records its subtree
 * carries; tau[6 + j] = a_j . moment of body j + 1, tau[0:6] = the base's force and moment.  A moment taken about the base and shifted back
 * would cancel two numbers a hundred times the result in float32.
 *
 * The root position never enters: an env 640 m out gets the bits of the same state at the origin.  There is no non-finite guard: a
 * non-finite input gives non-finite output for that env only.  Every call writes every word of the outputs it was given.  bias of a state
 * whose velocities are all zero equals gravity, and tau with accel = 0 equals bias, number for number (a zero's sign apart).
 *
 * The device table is dwj_pack_table's (include/dyros_jacobians.h), DWN_TABLE_WORDS = DWJ_TABLE_WORDS words; dwn_pack_table is that call under
 * this ABI's name and refuses what it refuses.
 */
#ifndef DYROS_DYNAMICS_H
#define DYROS_DYNAMICS_H

#include <stdint.h>

#include "dyros_jacobians.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DWN_ABI_VERSION 1

#define DWN_NUM_BODIES   38    /* Gym rigid bodies */
#define DWN_NUM_MOVING   34    /* floating base + 33 hinge links */
#define DWN_NUM_DOF      33
#define DWN_NUM_INERT    36    /* inertial records */
#define DWN_NV           39    /* generalised velocities: 6 + DWN_NUM_DOF */
#define DWN_MOM          6     /* words of a momentum row */
#define DWN_GROUP        4     /* envs per workgroup */
#define DWN_LANES        64    /* lanes per env */
#define DWN_TABLE_WORDS  1124  /* = DWJ_TABLE_WORDS */

int dwn_abi_version(void);
const char *dwn_last_error(void);
/* Host only, pure: dwj_pack_table under this ABI's name.  Writes table_host [DWN_TABLE_WORDS].  0, or -1 with the last error set. */
int dwn_pack_table(const DwjModel *m, uint32_t *table_host);
/* One launch on `stream`.  table [DWN_TABLE_WORDS], root_states [N,13] and dof_state [N,33,2] are device buffers; mass_scale [N,38],
 * dof_armature [N,33] and accel [N,39] are device buffers or NULL; (gx, gy, gz) is the gravity vector.  bias, gravity, tau [N,39] and
 * momentum [N,6] are device buffers or NULL.  No argument changes from call to call, nothing is allocated and nothing synchronises, so the call
 * sits inside a captured rollout step.  0, or -1 with the last error set; every refusal (num_envs < 1, a missing input, a table that is not
 * 16-byte aligned, tau without accel, no output at all, a non-finite gravity) happens before any launch. */
int dwn_inverse_dynamics(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *mass_scale,
                         const float *dof_armature, float gx, float gy, float gz, const float *accel, int32_t vel_at_com, float *bias,
                         float *gravity, float *tau, float *momentum, void *stream);

#ifdef __cplusplus
}
#endif

#endif
