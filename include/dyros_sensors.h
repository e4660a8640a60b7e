/* dyros_sensors.h -- C-ABI of the foot force-torque sensors (isaacgymdyros_amd/csrc/dw_sensors.hip): what
 * acquire_force_sensor_tensor / refresh_force_sensor_tensor give at the Gym boundary for sensors mounted on the two foot links,
 * [N, S, 6] = force then torque, and beside it the centre of pressure of each sole, the whole-body ZMP and the eight sole corners with
 * their ground reactions.  Opt-in and read-only: nothing here writes a buffer the step reads.
 *
 * What is measured.  The sole contact solve keeps its per-corner impulses [8][3] in the task record (DW_ES_WARM of dyros_walk.h;
 * corners 0..3 left sole, 4..7 right sole), written after every substep and zeroed when the env resets.  On the ground plane they are
 * world-frame impulses, so with inv_dt = 1 / dt (formed in float, 1.0f / (float)dt, as the step forms the factor it multiplies the sole
 * force by)
 *   f_k = WARM[k] * inv_dt          the force the ground exerts on corner k, world axes, over the LAST substep of the step
 * and sum_k f_k over a foot's corners is what the step adds into that foot's row of contact_forces.
 *
 * The foot pose x_f, R_f is the pose of moving body foot_mv[f] at the CURRENT (post-step) state, from root_states and dof_state by the chain
 * of dyros_bodies.h (the same table, the same link arithmetic), o_f = x_f - x_0 its offset from the base; c_k = foot_pos[k] is corner k in
 * the foot frame.  The choice of pose: lever arms are taken at the current pose, not at the pre-substep pose the solver used.  The two
 * differ by one substep of foot motion, which is nil in stance.
 *
 * sensors [N, S, 6], Gym's order, force then torque: the wrench the ground exerts on the foot through the sole solve, about the sensor's
 * origin.  Sensor s sits on foot f = foot_s at pos_s, quat_s (xyzw) in the foot frame:
 *   F_w = sum_k f_k                                  over the foot's four corners in index order
 *   T_w = sum_k (R_f (c_k - pos_s)) x f_k
 *   row = R(quat_s)^T R_f^T F_w, R(quat_s)^T R_f^T T_w          or F_w, T_w themselves where world_frame != 0
 * quat_s is used as given, R(quat_s) by the physics' quat_to_mat: the caller hands a unit quaternion (the Python layer normalises in double).
 * cop [N, 2, 4], per sole, in the FOOT frame (so independent of the pose): with n_k = f_k,z (never negative on the plane)
 *   words 0, 1 = sum_k n_k c_k,xy / sum_k n_k;  word 2 = Fz = sum_k n_k;  word 3 = the number of corners with n_k > 0, as a float.
 *   Where sum_k n_k is not above 0, all four words are 0.
 * zmp [N, 4]: words 0, 1 = world x, y of sum_k n_k p_k / sum_k n_k over all eight corners, p_k = x_f + R_f c_k, formed as an offset from
 *   the base with the base added last, one rounding (an env 640 m out is as accurate as env 0, dyros_bodies.h); word 2 = the total Fz;
 *   word 3 = the number of loaded corners.  All zero when nothing is loaded.
 * corners [N, 8, 6]: p_k (world, the base added last) and f_k (world): what a viewer draws the ground reaction from.
 *
 * What is NOT measured:
 *   - forces on the foot that do not come from the sole solve: self-collision capsules and the penalty contacts of other primitives
 *     (they are in the foot's row of contact_forces, not here);
 *   - gravity and joint forces (Gym: enable_forward_dynamics_forces = False, enable_constraint_solver_forces = True);
 *   - an env that was reset in the step's launch reads zero: the record's impulses were zeroed with it;
 *   - there is no non-finite guard: a NaN stays in its env's rows.
 *
 * Plane only.  On a height field the record holds impulses in each corner's contact frame (t1, t2, n), sampled at the pre-substep pose.
 * That frame is not kept, and sampling it again at the new pose is not the same thing across a cell edge, so the rows would be wrong
 * there without saying so.  The library cannot see the terrain; the Python layer refuses a cfg with terrain.  The follow-up: the step
 * would have to keep world-frame impulses in the record.
 */
#ifndef DYROS_SENSORS_H
#define DYROS_SENSORS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWF_ABI_VERSION 1

#define DWF_MAX_SENSORS   8
#define DWF_NUM_FEET      2
#define DWF_NUM_CORNERS   8     /* 0..3 left sole, 4..7 right sole */
#define DWF_SENSOR_WORDS  6     /* force, torque */
#define DWF_COP_WORDS     4     /* x, y (foot frame), Fz, loaded corners */
#define DWF_ZMP_WORDS     4     /* x, y (world), Fz, loaded corners */
#define DWF_CORNER_WORDS  6     /* p_k (world), f_k (world) */
#define DWF_LEG_DOF       12    /* the joints read: the first 24 words of a dof_state row; foot_mv must be in 1..12 */
#define DWF_DOF_ROW       66    /* words of a dof_state row */
#define DWF_ES_WORDS      372   /* = DW_ES_WORDS: words of an env_state row */
#define DWF_ES_WARM       344   /* = DW_ES_WARM */
#define DWF_WARM_WORDS    24
#define DWF_GROUP         16    /* envs per workgroup */

typedef struct DwfModel {
    int32_t foot_mv[DWF_NUM_FEET];          /* moving body of the left and of the right foot */
    float   foot_pos[DWF_NUM_CORNERS][3];   /* the corners in the foot frame, as DwModel.foot_pos */
    float   inv_dt;                         /* 1.0f / (float)dt of a physics substep */
} DwfModel;

typedef struct DwfSensor {
    int32_t foot;         /* 0 left, 1 right */
    float   pos[3];       /* in the foot frame */
    float   quat[4];      /* xyzw, in the foot frame */
    int32_t world_frame;
} DwfSensor;

int dwf_abi_version(void);
const char *dwf_last_error(void);
/* One launch on `stream`.  table [DWB_TABLE_WORDS] (dwb_pack_table's, 16-byte aligned), root_states [N,13], dof_state [N,33,2] and
 * env_state [N,DWF_ES_WORDS] (16-byte aligned) are device buffers; model_host and sensors_host [ns] are HOST memory, copied into the
 * kernel's argument block.  sensors [N, ns, 6] (NULL when ns is 0), cop [N,2,4], zmp [N,4], corners [N,8,6]: each may be NULL, at least
 * one must be given; any alignment of 4 bytes.  No argument changes from call to call, nothing is allocated and nothing synchronises, so
 * the call sits inside a captured rollout step.  0, or -1 with dwf_last_error() set; every refusal (num_envs < 1, a missing buffer, ns
 * outside 0..8, ns > 0 without sensors or the reverse, a foot outside 0..1, a quaternion whose norm is outside [0.99, 1.01], a non-finite
 * inv_dt, a foot_mv outside 1..12, no output) happens before any launch. */
int dwf_refresh(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const float *env_state,
                const DwfModel *model_host, const DwfSensor *sensors_host, int32_t ns, float *sensors, float *cop, float *zmp,
                float *corners, void *stream);

#ifdef __cplusplus
}
#endif

#endif
