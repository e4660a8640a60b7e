/* dyros_height_scan.h -- C-ABI of the terrain height scan (isaacgymdyros_amd/csrc/dw_height_scan.hip): the heights of
 * the ground at a yaw-aligned grid of points around the base, which is what the reference's terrain task feeds its policy
 * (tasks/anymal_terrain.py init_height_points / get_heights :501-536, the observation line :301-302), and the clearance over the ground of
 * points fixed to bodies, by default the eight sole corners the contact solve samples.  One launch, computed from the bound root_states
 * [N,13], dof_state [N,33,2] and height_samples (int16 [rows, cols], rows along x).  Opt-in and read-only: nothing here writes a buffer the
 * step reads.
 *
 * The map.  World x of sample line i is i * hscale - border, world y of sample line j likewise; the height of a sample is hs[i][j] * vscale.
 * hscale, vscale and border are DwConfig.terrain_hscale / terrain_vscale / terrain_border.  height_samples NULL is the ground plane.
 * A map side holds at most 8192 samples: beyond that terrain_sample's own upper clamp, (float)(rows - 1) - 1e-3f, no longer lies below the
 * last sample line in float32.
 *
 * Grid points.  P offsets (ox, oy) in metres in the base's yaw frame, 1 <= P <= DWH_MAX_POINTS, the same for every env.  DWH_MAX_POINTS is
 * 1024, a 32 x 32 grid: seven times the reference's 140 points (x = 0.1 * [-8..-2, 2..8], y = 0.1 * [-5..-1, 1..5], x-major as
 * meshgrid(x, y) flattens), while the offsets stay 8 KB of the table, which the kernel keeps in LDS beside the group's rows.
 *
 * Rule DWH_RULE_NEAREST is the reference's get_heights.  Every operation is float32 and rounded on its own (the sources are built with
 * -ffp-contract=off), in this order, (qx, qy, qz, qw) and (root_x, root_y) being words 3..6 and 0..1 of the root row:
 *   1. the yaw quaternion   n = sqrtf(qz * qz + qw * qw);  n = max(n, 1e-9f);  z = qz / n;  w = qw / n
 *                           (the reference's quat_apply_yaw: x and y zeroed, then normalize)
 *   2. the rotated offset   tx = -(z * oy) * 2;  ty = (z * ox) * 2;  X = (ox + w * tx) - z * ty;  Y = (oy + w * ty) + z * tx
 *                           (quat_apply with the terms that are zero dropped, which changes no bit)
 *   3. the world point      xw = X + root_x;  yw = Y + root_y
 *   4. the grid coordinate  gpu_div == 0:  u = (xw + border) / hscale            (CPU torch dividing a tensor by a Python scalar)
 *                           gpu_div != 0:  u = (xw + border) * (1.0f / hscale)   (torch-ROCm; the distinction DwConfig.torch_gpu_div makes)
 *                           v from yw likewise
 *   5. the index            u clamped in float to [0, rows - 2], then i = (int)u; j from v and cols likewise.  For every finite u this
 *                           equals the reference's truncate-then-clip, and no value outside int's range is ever converted.
 *   6. the height           h = min(hs[i][j], hs[i+1][j+1]) as int16;  height = (float)h * vscale
 *
 * Rule DWH_RULE_BILINEAR: (xw, yw) of steps 1..3, then terrain_sample of csrc/dw_physics.h itself (its own coordinate, clamp and bilinear
 * patch): the height the contact solve would see at that point.
 *
 * Probes.  B points fixed to bodies, 0 <= B <= DWH_MAX_PROBES: a Gym body and a point c in its frame.  The pose of the carrying moving body
 * m comes from the physics' own chain exactly as dyros_bodies.h states it (the base quaternion divided by its norm, offsets from the base
 * accumulated on their own), and
 *   probe_pos    = root[0:3] + (off_m + R_m c)          the base added last, one rounding
 *   (h, frame)   = terrain_sample(pos_x, pos_y)
 *   probe_height = h;  clearance = pos_z - h;  probe_normal = frame[6:9]
 * The contact solve's own depth measure of a sole corner is (pos_z - h) * normal_z, the vertical gap projected on the patch's normal
 * (dw_oct.h, dw_limb.h): clearance * probe_normal[2] is that number, and the two agree in sign everywhere.
 *
 * Ground plane (height_samples NULL): heights, probe_height +0.0, normals (0, 0, 1), clearance = pos_z, nothing of the map's arguments read:
 * the reference's get_heights on 'plane'.
 *
 * obs = clip(root_z - offset - height, -c, c) * scale: the reference's line 302 with offset, c and scale the table's (DwhParams.obs_*):
 *   d = (root_z - offset) - height;  d = d < -c ? -c : (d > c ? c : d);  obs = d * scale
 *
 * Guards.  No index is formed from a value that has not been clamped in float first; a point outside the map reads the clamped edge cell.
 * An env whose root row (13 words) or joint angles (33 words) are not all finite gets NaN in every float output, and reads nothing
 * of the map; no other env is affected.  There is no other guard.
 *
 * Exact properties (tested): root z, pitch and roll never enter `heights` or `points`; an env 640 m out gets the bits of the same state moved
 * there on a field with that period, when the shift is exact in float32; P changes no point's bits; an output that is not requested is
 * not written; the env's run is the same bits with the feature on or off.
 *
 * The device table.  dwh_pack_table validates on the host and writes DWH_TABLE_WORDS 32-bit words (integers or the bits of floats), which
 * the caller uploads as an ordinary tensor.  Layout:
 *   [0, DWB_TABLE_WORDS)      dwb_pack_table's words (dyros_bodies.h): the chain
 *   DWH_T_NP, DWH_T_NB, DWH_T_NW   P, B, and the number of walks (distinct carriers of the probes)
 *   DWH_T_ROWS .. DWH_T_BORDER     the map the table was packed for: rows, cols, hscale, vscale, border (rows = cols = 0: the plane)
 *   DWH_T_OBS                      obs_offset, obs_clip, obs_scale
 *   DWH_T_WALK  [DWH_MAX_PROBES][2]                 a walk: the root-to-leaf path, and how many of its bodies lead to the carrier
 *   DWH_T_PROBE [DWH_MAX_PROBES][DWH_PROBE_WORDS]   Gym body, walk, c[3]  (a probe on the base takes a walk of depth 0)
 *   DWH_T_GRID  [DWH_MAX_POINTS][2]                 ox, oy
 */
#ifndef DYROS_HEIGHT_SCAN_H
#define DYROS_HEIGHT_SCAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWH_ABI_VERSION 1

#define DWH_MAX_POINTS   1024  /* grid points: a 32 x 32 grid */
#define DWH_MAX_PROBES   16
#define DWH_GROUP        16    /* envs per workgroup */
#define DWH_LANES        16    /* lanes per env (the workgroup's 256 lanes then run across the group's points) */
#define DWH_RULE_NEAREST  0
#define DWH_RULE_BILINEAR 1

#define DWH_PROBE_WORDS  5
#define DWH_T_CHAIN      0
#define DWH_T_NP         772   /* = DWB_TABLE_WORDS */
#define DWH_T_NB         773
#define DWH_T_NW         774
#define DWH_T_ROWS       775
#define DWH_T_COLS       776
#define DWH_T_HSCALE     777
#define DWH_T_VSCALE     778
#define DWH_T_BORDER     779
#define DWH_T_OBS        780
#define DWH_T_WALK       784
#define DWH_T_PROBE      816
#define DWH_T_GRID       896
#define DWH_TABLE_WORDS  2944

typedef struct DwhProbe {
    int32_t body;          /* Gym body id */
    float pos[3];          /* the point, in the body's frame */
} DwhProbe;

typedef struct DwhParams {
    int32_t rows, cols;                      /* the map; 0, 0: the ground plane (hscale, vscale and border are then not looked at) */
    float hscale, vscale, border;
    float obs_offset, obs_clip, obs_scale;
} DwhParams;

int dwh_abi_version(void);
const char *dwh_last_error(void);
/* Host only, pure: validates and writes table_host [DWH_TABLE_WORDS].  model: a DwbModel (dyros_bodies.h); grid_xy [np][2]; probes [nb] or
 * NULL with nb 0.  Refuses what dwb_pack_table refuses, np outside 1..DWH_MAX_POINTS, nb outside 0..DWH_MAX_PROBES, an offset, a point or a
 * parameter that is not finite, hscale or vscale not finite and > 0, a map smaller than 2 x 2 (other than 0 x 0) or with a side of more than 8192
 * samples, obs_clip < 0, a probe on an unknown body.  0, or -1 with dwh_last_error() set. */
int dwh_pack_table(const void *model, const float *grid_xy, int32_t np, const DwhProbe *probes, int32_t nb, const DwhParams *params,
                   uint32_t *table_host);
/* One launch on `stream`.  table [DWH_TABLE_WORDS], root_states, dof_state and height_samples (int16 [rows][cols], or NULL: the plane) are
 * device buffers; P and B are the table's (the outputs are sized by them; with B = 0 the probe outputs are not touched).  rule: DWH_RULE_*.
 * Outputs, each or NULL, at least one given: heights [N,P], points [N,P,2] (xw, yw), obs [N,P], probe_pos [N,B,3], probe_height [N,B],
 * clearance [N,B], probe_normal [N,B,3].  No argument changes from call to call, nothing is allocated and nothing synchronises, so the call
 * sits inside a captured rollout step.  0, or -1 with dwh_last_error() set; every refusal (num_envs < 1, a missing buffer, a misaligned
 * table, a map smaller than 2 x 2 or with a side of more than 8192 samples, hscale or vscale not finite and > 0, a border that is not finite, an unknown
 * rule, no output) happens before any launch. */
int dwh_scan(int32_t num_envs, const uint32_t *table, const float *root_states, const float *dof_state, const int16_t *height_samples,
             int32_t rows, int32_t cols, float hscale, float vscale, float border, int32_t rule, int32_t gpu_div, float *heights,
             float *points, float *obs, float *probe_pos, float *probe_height, float *clearance, float *probe_normal, void *stream);

#ifdef __cplusplus
}
#endif

#endif
