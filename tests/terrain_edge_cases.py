"""Height-field scenes at the edges of the map, of the sample grid and of the coarse bound table, shared by the CPU tests
(tests/test_terrain_edges.py: host emulation of the kernel source) and the GPU tests (tests/test_terrain_edges_gpu.py: the HIP
library): a scene = a hand-made field + a seeded state + joint torques, run for ONE substep through dw_simulate and compared with
the oracle, which samples the field under every primitive and has no table.  Test helper, in the style of tests/knob_cases.py.

Tolerances (none derived from a kernel):
  * loaded bodies: the same (env, body) pairs carry more than 1 N; a pair is left out only if the oracle's norm is within the force
    tolerance of 1 N;
  * net contact forces: 2e-3 max|F| + 0.05 (the rule of the two terrain tests of tests/test_hip_gpu.py);
  * positions (root pose, q): 1e-5 against the fp32 oracle;
  * velocities (root velocity, qd, one figure for all 39): 1e-5 against the fp32 oracle where that is met, otherwise against the fp64
    oracle within FP64_FACTOR = 4 x the fp32-to-fp64 oracle difference of the scene, computed here (tests/knob_cases.py's rule);
  * every output finite.

Beside the scenes stands a restatement in numpy of the coarse bound table (dw_physics.h terrain_bound_cell / terrain_bound) with
`cell` and `reach` as parameters, and with the ways it could be wrong as parameters too (no reach window, a window cut on one side,
rows taken for cols): the table has no export, so what is asserted is (a) the invariant on the oracle's own data -- no body the oracle
loads has its origin higher above the bound of its robot's cell than its bounding radius -- and (b) that the scenes BITE: with a wrong
table the same data break the invariant, i.e. a kernel with that table would drop contacts the oracle reports.
"""
import ctypes as C

import numpy as np

from isaacgymdyros_amd.model import load_model
from isaacgymdyros_amd.task_constants import INITIAL_DOF_POS
from isaacgymdyros_amd.terrain import TerrainCfg
from oracle.oracle import OracleSim

MODEL = load_model()
STATE_TOL, FP64_FACTOR, LOADED_N = 1e-5, 4.0, 1.0
HM_CELL, HM_MARGIN = 0.5, 0.05                      # dw_physics.h
FEET = (MODEL.left_foot_idx, MODEL.right_foot_idx)
Q0 = np.asarray(INITIAL_DOF_POS, np.float64)
f32 = np.float32


# ---------------------------------------------------------------------------------------------- the field
class Field:
    """A hand-made height field with the attributes OracleSim / EmulSim / HipSim(terrain=...) read."""

    def __init__(self, samples, hscale=0.1, vscale=0.005, border=2.0):
        self.heightsamples = np.ascontiguousarray(samples, dtype=np.int16)
        assert np.array_equal(self.heightsamples, np.asarray(samples))          # (fits int16)
        self.tot_rows, self.tot_cols = self.heightsamples.shape
        self.hscale, self.vscale, self.border = float(hscale), float(vscale), float(border)
        self.env_length = 8.0
        self.env_origins = np.zeros((1, 1, 3))
        self.cfg = TerrainCfg(mesh_type="heightfield", horizontal_scale=hscale, vertical_scale=vscale, border_size=border,
                              curriculum=False, num_rows=1, num_cols=1)

    @property
    def extent(self):
        """World coordinates of sample 0 and of the last sample line, per axis: ((x0, x1), (y0, y1))."""
        return ((-self.border, (self.tot_rows - 1) * self.hscale - self.border), (-self.border, (self.tot_cols - 1) * self.hscale - self.border))

    def uv(self, x, y):
        """Grid coordinates of world points BEFORE the clamps, in the kernels' arithmetic: fp32, (x + border) * (1 / hscale)."""
        inv = f32(1.0) / f32(self.hscale)
        return (f32(x) + f32(self.border)) * inv, (f32(y) + f32(self.border)) * inv

    def clamped(self, u, v):
        umax, vmax = f32(self.tot_rows - 1) - f32(1e-3), f32(self.tot_cols - 1) - f32(1e-3)
        return np.clip(u, f32(0), umax), np.clip(v, f32(0), vmax)

    def height_at(self, x, y):
        """Bilinear height in float64, with the clamps of terrain_sample."""
        u = np.clip((np.asarray(x, np.float64) + self.border) / self.hscale, 0.0, self.tot_rows - 1 - 1e-3)
        v = np.clip((np.asarray(y, np.float64) + self.border) / self.hscale, 0.0, self.tot_cols - 1 - 1e-3)
        i, j = u.astype(int), v.astype(int)
        a, b = u - i, v - j
        h = self.heightsamples.astype(np.float64)
        return self.vscale * ((1 - a) * ((1 - b) * h[i, j] + b * h[i, j + 1]) + a * ((1 - b) * h[i + 1, j] + b * h[i + 1, j + 1]))


# ---------------------------------------------------------------------------------------------- kinematics in numpy (float64)
def _quat_to_mat(q):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def fk(root, q):
    """World position [N, 34, 3] and rotation [N, 34, 3, 3] of every moving body: R_b = R_parent rot0_b Rot(axis_b, q_b),
    x_b = x_parent + R_parent pos_b (the chain of oracle/dw_amp.c dwo_body_positions, which test_fk_agrees_with_the_oracle holds it to)."""
    root, q = np.asarray(root, np.float64), np.asarray(q, np.float64)
    N, nb = len(root), len(MODEL.mv_parent)
    x, R = np.zeros((N, nb, 3)), np.zeros((N, nb, 3, 3))
    x[:, 0], R[:, 0] = root[:, :3], _quat_to_mat(root[:, 3:7] / np.linalg.norm(root[:, 3:7], axis=1, keepdims=True))
    for b in range(1, nb):
        p = MODEL.mv_parent[b]
        k, ang = np.asarray(MODEL.mv_axis[b]), q[:, b - 1]
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        rot = np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)
        x[:, b] = x[:, p] + R[:, p] @ np.asarray(MODEL.mv_pos[b])
        R[:, b] = R[:, p] @ np.asarray(MODEL.mv_rot0[b]) @ rot
    return x, R


def sole_corners(root, q):
    """World positions [N, 8, 3] of the sole corners: the contact points of the two foot bodies."""
    x, R = fk(root, q)
    return np.stack([x[:, f["moving"]] + R[:, f["moving"]] @ np.asarray(f["pos"]) for f in MODEL.foot_pts], 1)


GROUND_GEOMS = [g for g in MODEL.geoms if not g["sole"]]


def ground_points(root, q):
    """World positions [N, primitives, 3] of the ONE point of every ground primitive that the physics tests against the ground: the
    deepest corner of a box, the lowest point of the lower cap's rim of a cylinder (oracle/dw_physics.c, section on geoms)."""
    x, R = fk(root, q)
    out = np.zeros((len(x), len(GROUND_GEOMS), 3))
    for n, g in enumerate(GROUND_GEOMS):
        b, rot, pos, size = g["moving"], np.asarray(g["rot"]), np.asarray(g["pos"]), np.asarray(g["size"])
        Rw = R[:, b]
        if g["type"] == 0:
            e = np.where((Rw @ rot)[:, 2, :] > 0, -1.0, 1.0) * size
            out[:, n] = x[:, b] + (Rw @ (rot @ e[:, :, None] + pos[:, None]))[:, :, 0]
        else:
            aw = Rw @ rot[:, 2]
            sgn = np.where(aw[:, 2] >= 0, -1.0, 1.0)[:, None]
            dw = np.array([0, 0, 1.0]) - aw[:, 2:3] * aw
            dn = np.linalg.norm(dw, axis=1, keepdims=True)
            off = np.where(dn > 1e-6, -size[0] / np.maximum(dn, 1e-6) * dw, 0.0)
            out[:, n] = x[:, b] + (Rw @ (pos + sgn * size[1] * rot[:, 2])[:, :, None])[:, :, 0] + off
    return out


def oracle_body_origins(sim):
    """[N, 34, 3] from the oracle's body-position entry point (at most DW_MAX_BODY_QUERY = 8 bodies per call)."""
    nb = len(MODEL.mv_parent)
    out = np.zeros((sim.N, nb, 3), np.float32)
    for b0 in range(0, nb, 8):
        ids = list(range(b0, min(b0 + 8, nb)))
        arr, part = (C.c_int32 * len(ids))(*ids), np.zeros((sim.N, len(ids), 3), np.float32)
        assert sim.api["body_positions"](sim.h, arr, len(ids), part.ctypes.data_as(C.c_void_p), None) == 0
        out[:, ids] = part
    return out


def body_radii():
    """Per moving body the bounding radius of its ground primitives about the body origin, offset + extent per primitive as
    dw_physics.h model_reach has it (0 for a body without one; the sole boxes are no ground primitives: their corners are sampled
    unconditionally).  The kernels test against 1.01 x this + 1 mm, so an invariant that holds with this radius holds with theirs."""
    r = np.zeros(len(MODEL.mv_parent))
    for g in MODEL.geoms:
        if g["sole"]:
            continue
        s = g["size"]
        ext = np.linalg.norm(s[:3]) if g["type"] == 0 else np.hypot(s[0], s[1])
        r[g["moving"]] = max(r[g["moving"]], np.linalg.norm(g["pos"]) + ext)
    return r


def model_reach():
    """dw_physics.h model_reach: chain of link offsets to the primitive's body + the primitive's farthest point + margin (TOCABI 1.43 m)."""
    chain = np.zeros(len(MODEL.mv_parent))
    for b in range(1, len(chain)):
        chain[b] = chain[MODEL.mv_parent[b]] + np.linalg.norm(MODEL.mv_pos[b])
    best = 0.0
    for g in MODEL.geoms:
        s = g["size"]
        ext = np.linalg.norm(s[:3]) if g["type"] == 0 else np.hypot(s[0], s[1])
        best = max(best, chain[g["moving"]] + np.linalg.norm(g["pos"]) + ext)
    return best + HM_MARGIN


# ---------------------------------------------------------------------------------------------- the bound table, restated
def cell_samples(hscale):
    return max(1, int(f32(HM_CELL) / f32(hscale)))


def reach_samples(hscale, reach=None):
    return int(f32(model_reach() if reach is None else reach) / f32(hscale)) + 2


def bound_table(hs, cell, reach, cut=None):
    """terrain_bound_cell for every cell: the largest sample of the cell's own samples widened by `reach` samples on every side,
    clipped to the map.  cut = "+x" / "-x" / "+y" / "-y": the window is NOT widened on that side (a wrong table, for the bite checks)."""
    rows, cols = hs.shape
    hr, hc = -(-rows // cell), -(-cols // cell)
    out = np.zeros((hr, hc), np.int16)
    for ci in range(hr):
        i0, i1 = ci * cell - (0 if cut == "-x" else reach), ci * cell + cell - 1 + (0 if cut == "+x" else reach)
        for cj in range(hc):
            j0, j1 = cj * cell - (0 if cut == "-y" else reach), cj * cell + cell - 1 + (0 if cut == "+y" else reach)
            out[ci, cj] = hs[max(i0, 0):min(i1, rows - 1) + 1, max(j0, 0):min(j1, cols - 1) + 1].max()
    return out


def bound_at(field, table, cell, x, y, swap=False):
    """terrain_bound: the table entry of the cell under world (x, y), index arithmetic of terrain_sample (fp32, clamps, (int)u / cell).
    swap: the table was built and is read with rows and cols exchanged (samples taken as [cols][rows], u clamped to cols, v to rows)."""
    u, v = field.uv(x, y)
    if swap:
        umax, vmax = f32(field.tot_cols - 1) - f32(1e-3), f32(field.tot_rows - 1) - f32(1e-3)
        u, v = np.clip(u, f32(0), umax), np.clip(v, f32(0), vmax)
    else:
        u, v = field.clamped(u, v)
    return field.vscale * table[u.astype(np.int32) // cell, v.astype(np.int32) // cell].astype(np.float64)


def swapped_table(field, cell, reach):
    """The table of a builder that took rows for cols: the same samples in memory read as [cols][rows]."""
    return bound_table(field.heightsamples.reshape(field.tot_cols, field.tot_rows), cell, reach)


def loaded_pairs(sim_or_forces):
    """(env, moving body, Gym body) of every pair the forces load above 1 N through a ground primitive (the foot bodies report the
    sole corners, which no table gates: left out)."""
    cf = sim_or_forces if isinstance(sim_or_forces, np.ndarray) else sim_or_forces.buf["contact_forces"]
    e, g = np.nonzero(np.linalg.norm(cf, axis=2) > LOADED_N)
    keep = ~np.isin(g, FEET)
    e, g = e[keep], g[keep]
    return e, np.asarray(MODEL.body_moving)[g], g


def above_bound(field, root, origins, pairs, table, cell, swap=False):
    """Per loaded pair: how far the body's origin is above the bound of its robot's cell, minus the body's bounding radius.  > 0:
    a kernel with this table skips the body."""
    e, mv, _ = pairs
    zb = bound_at(field, table, cell, root[:, 0], root[:, 1], swap=swap)
    return origins[e, mv, 2].astype(np.float64) - zb[e] - body_radii()[mv]


# ---------------------------------------------------------------------------------------------- scenes
def _rough(rng, rows, cols, vscale, amp=0.04):
    q = int(round(amp / vscale))
    return rng.integers(-q, q + 1, size=(rows, cols)).astype(np.int16)


def _ridge(hs, vscale, height=0.3):
    hs = hs.copy()
    k = int(round(height / vscale))
    hs[0, :] = hs[-1, :] = hs[:, 0] = hs[:, -1] = k
    return hs


def _yaw_quat(yaw, tilt=None):
    """Heading yaw, then a small tilt about the body's x and y axes: an exactly level box has no deepest corner, and which one a sign
    test picks is then decided by rounding -- on a height field the corners stand over different ground."""
    z = np.zeros_like(yaw)
    q = np.stack([z, z, np.sin(yaw / 2), np.cos(yaw / 2)], 1)
    if tilt is not None:
        t = np.stack([tilt[:, 0] / 2, tilt[:, 1] / 2, z, np.ones_like(yaw)], 1)
        x1, y1, z1, w1 = q.T
        x2, y2, z2, w2 = t.T
        q = np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                      w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], 1)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _standing(field, xy, quat, rng, depth=(0.0001, 0.004), q=None):
    """Robots on their soles at base (x, y) with heading yaw: the DEEPEST sole corner 0.1 .. 4 mm inside the ground under it (the field
    differs from corner to corner), joints within 0.02 rad of the initial pose unless given, small base and joint rates."""
    N = len(xy)
    root = np.zeros((N, 13))
    root[:, 0:2], root[:, 3:7] = xy, quat
    q = Q0 + rng.normal(size=(N, 33)) * 0.02 if q is None else q
    root32 = root.astype(f32).astype(np.float64)                      # the corners of the state the backends will get
    c = sole_corners(root32, q.astype(f32))
    gap = c[:, :, 2] - field.height_at(c[:, :, 0], c[:, :, 1])
    root[:, 2] = -gap.min(axis=1) - rng.uniform(depth[0], depth[1], N)
    root[:, 7:10] = rng.normal(size=(N, 3)) * 0.1
    root[:, 10:13] = rng.normal(size=(N, 3)) * 0.1
    dof = np.zeros((N, 33, 2))
    dof[:, :, 0], dof[:, :, 1] = q, rng.normal(size=(N, 33)) * 0.2
    return root.astype(f32), dof.astype(f32)


def _fallen(field, xy, rng):
    """The lying, kneeling and tumbling poses of test_fallen_robots_on_high_rough_terrain_touch_like_the_oracle at base (x, y)."""
    N = len(xy)
    root = np.zeros((N, 13))
    root[:, 0:2] = xy
    root[:, 2] = field.height_at(xy[:, 0], xy[:, 1]) + rng.uniform(0.12, 0.45, size=N)
    ax = rng.normal(size=(N, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(0.6, 3.0, size=N)
    root[:, 3:6], root[:, 6] = ax * np.sin(ang / 2)[:, None], np.cos(ang / 2)
    root[:, 7:13] = rng.normal(size=(N, 6)) * 0.2
    dof = np.zeros((N, 33, 2))
    dof[:, :, 0], dof[:, :, 1] = Q0 + rng.normal(size=(N, 33)) * 0.3, rng.normal(size=(N, 33)) * 0.5
    return root.astype(f32), dof.astype(f32)


def _tau(N, rng, amp=30.0):
    return rng.uniform(-amp, amp, size=(N, 33)).astype(f32)


def _borders(border, seed=31, N=128):
    """A1: a 70 x 90 map, +-40 mm per sample, a 0.3 m ridge on the outermost rows and columns (so the clamped edge differs from the
    interior).  Base x and y drawn independently from: sample 0, 0.3 m and 1.5 m outside on either side, the last sample line, 1e-4
    before it, just beyond it, and the interior."""
    rng = np.random.default_rng(seed)
    field = Field(_ridge(_rough(rng, 70, 90, 0.005), 0.005), 0.1, 0.005, border)
    xy = np.zeros((N, 2))
    for ax, (lo, hi) in enumerate(field.extent):
        spots = np.array([lo, lo - 0.3, lo - 1.5, hi + 0.3, hi + 1.5, hi, hi - 1e-4, hi + 0.05, np.nan])
        pick = spots[rng.integers(0, len(spots), size=N)]
        xy[:, ax] = np.where(np.isnan(pick), rng.uniform(lo + 0.5, hi - 0.5, size=N), pick)
    root, dof = _standing(field, xy, _yaw_quat(rng.uniform(-np.pi, np.pi, N), rng.uniform(-0.03, 0.03, (N, 2))), rng)
    return field, root, dof, _tau(N, rng)


def line_floats(field, k, axis):
    """World coordinates (fp32) around sample line k of an axis: the largest float whose grid coordinate u, in the kernels' arithmetic,
    is below k, one whose u is exactly k (None if no float gives it), and the smallest with u above k."""
    inv, b = f32(1.0) / f32(field.hscale), f32(field.border)
    u = lambda x: (f32(x) + b) * inv
    x = f32(np.float64(k) * field.hscale - field.border)
    while u(x) >= k:
        x = np.nextafter(x, f32(-np.inf))
    below = x
    x = np.nextafter(x, f32(np.inf))
    on = x if u(x) == k else None
    while u(x) <= k:
        x = np.nextafter(x, f32(np.inf))
    return below, on, x


def _lines(seed=32, N=126):
    """A2: a 60 x 80 map at 0.1 m (bound cells of 5 samples): ONE plane, 15 mm up per row and 10 mm down per column.  (Across a sample
    line the bilinear height is continuous but its gradient is not, so over rough ground a contact point ON a line gets one of two
    normals by the last bit of its coordinate: the fp32 and fp64 oracles themselves then differ by 0.3 rad/s, measured with +-40 mm
    per sample.  On a plane either side gives the same answer, a row taken for a column or a patch read one sample off does not.)  Per axis and env a sample line k, every other one a
    bound-cell line (k a multiple of 5), and one of three places: the float just below the line, the float on it, the float just above.
    A third of the envs put the BASE there; the others, heading along an axis, put a sole corner there (to within the rounding of the
    chain to the foot, so those corners fall on either side of the line and on it)."""
    rng = np.random.default_rng(seed)
    field = Field(3 * np.arange(60)[:, None] - 2 * np.arange(80)[None, :], 0.1, 0.005, 2.0)
    q = Q0 + rng.normal(size=(N, 33)) * 0.02
    quat = _yaw_quat(rng.integers(0, 4, size=N) * (np.pi / 2), rng.uniform(-0.03, 0.03, (N, 2)))
    what = np.arange(N) % 3                                               # 0: the base on the line, 1 / 2: a sole corner
    corner = rng.integers(0, 8, size=N)
    root0 = np.zeros((N, 7)); root0[:, 3:7] = quat
    off = sole_corners(root0.astype(f32), q.astype(f32))[np.arange(N), corner, :2]      # corner relative to the base
    xy = np.zeros((N, 2), f32)
    for ax, n in enumerate((field.tot_rows, field.tot_cols)):
        for e in range(N):
            k = 20
            while abs(k * field.hscale - field.border) < 0.25:           # (world 0 is left out: the floats there are 1e7 times denser than u's)
                k = int(rng.integers(2, (n - 2) // 5)) * 5 if rng.integers(0, 2) else int(rng.integers(8, n - 8))
            cand = [c for c in line_floats(field, k, ax) if c is not None]
            x = cand[int(rng.integers(0, len(cand)))]
            xy[e, ax] = x if what[e] == 0 else f32(np.float64(x) - off[e, ax])
    root, dof = _standing(field, xy.astype(np.float64), quat, rng, q=q)
    root[:, 0:2] = xy                                                     # (bit for bit the floats chosen above)
    return field, root, dof, _tau(N, rng)


SCALES = {"h0.07": (0.07, 0.005, 101, 87), "h0.25": (0.25, 0.02, 33, 27), "h0.5": (0.5, 0.005, 21, 17), "h1.0": (1.0, 0.02, 12, 9)}


def _scales(name, seed=33, N=96):
    """A3: another horizontal scale -- 0.07 (cells of 7 samples), 0.25 (2), 0.5 (1), 1.0 ((int)0.5 = 0, floored to 1) -- with vertical
    scales 0.005 and 0.02, on maps whose row and column counts are no multiples of the cell and differ from each other; heights +-0.3 x
    the sample spacing (at most +-40 mm); robots over the whole map, the partial last cells and a margin outside included."""
    hscale, vscale, rows, cols = SCALES[name]
    rng = np.random.default_rng(seed + int(hscale * 100))
    field = Field(_rough(rng, rows, cols, vscale, amp=min(0.04, 0.3 * hscale)), hscale, vscale, 1.0)
    (x0, x1), (y0, y1) = field.extent
    xy = np.stack([rng.uniform(x0 - 0.3, x1 + 0.3, N), rng.uniform(y0 - 0.3, y1 + 0.3, N)], 1)
    cell = cell_samples(hscale)
    last = N // 3                                                          # a third of them in the partial last row / column of cells
    xy[:last:2, 0] = rng.uniform(((rows - 1) // cell) * cell * hscale - 1.0, x1, len(xy[:last:2]))
    xy[1:last:2, 1] = rng.uniform(((cols - 1) // cell) * cell * hscale - 1.0, y1, len(xy[1:last:2]))
    root, dof = _standing(field, xy, _yaw_quat(rng.uniform(-np.pi, np.pi, N), rng.uniform(-0.03, 0.03, (N, 2))), rng)
    return field, root, dof, _tau(N, rng)


# arm poses of A4 (left arm; the right arm mirrors every angle), the eight joints from Shoulder1 to Wrist2: all zero is the arm straight
# out sideways at shoulder height, Shoulder1 swings it forward in the horizontal plane
ARM_SPREAD = np.zeros(8)
ARM_FORWARD = np.array([-1.2, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
ARM_BODIES = (19, 21, 23, 29, 31, 33)                                      # moving bodies: upper arm, forearm, hand of either arm
PILLAR = 5.0                                                              # height of pillars and walls [m]: far above the raised hands


def _walls(seed=34, N=128):
    """A4: a flat floor at 0 on a 120 x 90 map with six pillars 5 m tall, one sample wide or a wall of three samples: a bilinear tent
    +-0.1 m around each, 3.9 m and 4.3 m apart, so that no robot has two of them in reach.  Robots stand on the floor, arms spread or
    reaching forward (drawn around ARM_SPREAD / ARM_FORWARD), heading within 0.3 rad of +x, -x, +y or -y, placed so that the tested
    point of one primitive of an upper arm, a forearm or a hand, 0.3 .. 0.9 m from the base, lies within 30 mm of a pillar's sample:
    inside the tent.  The floor under the base is 0, so only the reach window of the bound table knows about the pillar."""
    rng = np.random.default_rng(seed)
    hs = np.zeros((120, 90), np.int16)
    top = int(round(PILLAR / 0.005))
    pillars = [(i, j) for i in (20, 59, 98) for j in (22, 65)]                           # rows 0, 4, 3 and columns 2, 0 modulo the cell size 5
    for n, (i, j) in enumerate(pillars):
        hs[i, j] = top
        if n % 3 == 1:
            hs[i - 1:i + 2, j] = top
        if n % 3 == 2:
            hs[i, j - 1:j + 2] = top
    field = Field(hs, 0.1, 0.005, 2.0)
    M = 2 * N                                                                             # candidates: those with a foot on a tent leave
    q = Q0 + rng.normal(size=(M, 33)) * 0.02
    pose = np.where((rng.integers(0, 2, size=M) == 0)[:, None], ARM_SPREAD, ARM_FORWARD) + rng.uniform(-0.15, 0.15, size=(M, 8))
    q[:, 15:23], q[:, 25:33] = pose, -pose
    quat = _yaw_quat(rng.integers(0, 4, size=M) * (np.pi / 2) + rng.uniform(-0.3, 0.3, M), rng.uniform(-0.03, 0.03, (M, 2)))
    root0 = np.zeros((M, 7)); root0[:, 3:7] = quat
    pts = ground_points(root0.astype(f32), q.astype(f32))
    dist = np.linalg.norm(pts[:, :, :2], axis=2)
    arm = np.array([g["moving"] in ARM_BODIES for g in GROUND_GEOMS])
    ok = arm[None, :] & (dist >= 0.3) & (dist <= 0.9)
    assert ok.any(axis=1).all()
    which = np.array([rng.choice(np.nonzero(row)[0]) for row in ok])
    touch = pts[np.arange(M), which]
    pick = np.asarray(pillars)[rng.integers(0, len(pillars), size=M)]
    pxy = pick * 0.1 - 2.0 + rng.uniform(-0.03, 0.03, size=(M, 2))
    root, dof = _standing(field, pxy - touch[:, :2], quat, rng, q=q)
    keep = np.nonzero(root[:, 2] < 0.95)[0][:N]                                           # both feet on the floor
    assert len(keep) == N
    return field, root[keep], dof[keep], _tau(N, rng, amp=10.0)


def _fallen_at_the_edge(seed=35, N=96):
    """A5: the lying and tumbling poses of the fallen-robots test on the A1 field, bases within 0.5 m of the map's outline on either
    side of it."""
    rng = np.random.default_rng(seed)
    field = Field(_ridge(_rough(rng, 70, 90, 0.005), 0.005), 0.1, 0.005, 2.0)
    (x0, x1), (y0, y1) = field.extent
    side, along, d = rng.integers(0, 4, size=N), rng.uniform(0, 1, N), rng.uniform(-0.5, 0.5, N)
    xy = np.zeros((N, 2))
    xy[:, 0] = np.select([side == 0, side == 1], [x0 + d, x1 + d], x0 + along * (x1 - x0))
    xy[:, 1] = np.select([side == 2, side == 3], [y0 + d, y1 + d], y0 + along * (y1 - y0))
    root, dof = _fallen(field, xy, rng)
    return field, root, dof, np.zeros((N, 33), f32)


SCENES = {"borders": lambda: _borders(2.0), "borders_no_border": lambda: _borders(0.0), "lines": _lines,
          "scales_h0.07": lambda: _scales("h0.07"), "scales_h0.25": lambda: _scales("h0.25"), "scales_h0.5": lambda: _scales("h0.5"),
          "scales_h1.0": lambda: _scales("h1.0"), "walls": _walls, "fallen_at_the_edge": _fallen_at_the_edge}
_scenes, _oracle = {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = SCENES[name]()
    return _scenes[name]


# ---------------------------------------------------------------------------------------------- the runner and the checks
_OUT = ("root_states", "dof_state", "contact_forces")


def run_scene(make_sim, name):
    """One substep of the scene through dw_simulate of a backend: make_sim(N, terrain=field) -> OracleSim / EmulSim / HipSim."""
    field, root, dof, tau = scene(name)
    sim = make_sim(len(root), terrain=field)
    try:
        sim.buf["root_states"][...], sim.buf["dof_state"][...] = root, dof
        sim.buf["contact_forces"][...] = 0
        sim.simulate(tau)
        return {k: sim.buf[k].copy() for k in _OUT}
    finally:
        if hasattr(sim, "close"):
            sim.close()


def oracle_run(name, double=False):
    """The oracle's result of a scene (cached: every build asks), with the body origins of the scene's initial state."""
    if (name, double) not in _oracle:
        _oracle[name, double] = run_scene(lambda N, terrain: OracleSim(N, terrain=terrain, terrain_curriculum=0, double=double), name)
    return _oracle[name, double]


def ground_forces(name):
    """The oracle's contact forces of the scene with self-collision off: what the ground alone loads (the table gates nothing else)."""
    if ("ground", name) not in _oracle:
        _oracle["ground", name] = run_scene(lambda N, terrain: OracleSim(N, terrain=terrain, terrain_curriculum=0, self_collision=0), name)["contact_forces"]
    return _oracle["ground", name]


def initial_origins(name):
    if ("origins", name) not in _oracle:
        field, root, dof, _ = scene(name)
        sim = OracleSim(len(root), terrain=field, terrain_curriculum=0)
        sim.buf["root_states"][...], sim.buf["dof_state"][...] = root, dof
        _oracle["origins", name] = oracle_body_origins(sim)
    return _oracle["origins", name]


def _velocity_diff(a, b):
    return float(max(np.abs(a["root_states"][:, 7:] - b["root_states"][:, 7:]).max(), np.abs(a["dof_state"][..., 1] - b["dof_state"][..., 1]).max()))


def _position_diff(a, b):
    return float(max(np.abs(a["root_states"][:, :7] - b["root_states"][:, :7]).max(), np.abs(a["dof_state"][..., 0] - b["dof_state"][..., 0]).max()))


def compare(ref, ref64, got):
    """The figures of one result against the oracle's: what check() asserts and DESIGN.md section 4 tabulates."""
    cfa, cfb = ref["contact_forces"], got["contact_forces"]
    na, nb = np.linalg.norm(cfa, axis=2), np.linalg.norm(cfb, axis=2)
    ftol = 2e-3 * float(np.abs(cfa).max()) + 0.05
    decided = np.abs(na - LOADED_N) > ftol                                 # the oracle's norm is not within the force tolerance of 1 N
    o3264 = _velocity_diff(ref, ref64)
    return dict(finite=all(bool(np.isfinite(got[k]).all()) for k in _OUT), loaded=int((na > LOADED_N).sum()),
                loaded_mismatch=int((((na > LOADED_N) != (nb > LOADED_N)) & decided).sum()), fmax=float(np.abs(cfa).max()),
                force=float(np.abs(cfa - cfb).max()), force_tol=ftol, pos=_position_diff(ref, got), v32=_velocity_diff(ref, got),
                v64=_velocity_diff(ref64, got), o3264=o3264, v64_bound=FP64_FACTOR * o3264)


def check(name, got, label=""):
    """Holds a backend's result of a scene to the oracle's at the tolerances of this module's docstring; prints the figures first."""
    c = compare(oracle_run(name), oracle_run(name, double=True), got)
    print("%-20s %-10s loaded %d (mismatch %d) | forces %.3g of %.3g (peak %.3g N) | positions %.2e | velocities vs fp32 %.2e, vs fp64 %.2e "
          "(fp32 / fp64 oracles %.2e, bound %.2e)" % (name, label, c["loaded"], c["loaded_mismatch"], c["force"], c["force_tol"], c["fmax"],
                                                      c["pos"], c["v32"], c["v64"], c["o3264"], c["v64_bound"]))
    assert c["finite"], name
    assert c["loaded_mismatch"] == 0, (name, c)
    assert c["force"] <= c["force_tol"], (name, c)
    assert c["pos"] <= STATE_TOL, (name, c)
    assert c["v32"] <= STATE_TOL or c["v64"] <= c["v64_bound"], (name, c)
    return c


# ---------------------------------------------------------------------------------------------- what a scene reaches
def reach_counts(name):
    """Where the scene's contact points (the 8 sole corners and the tested point of each of the 59 ground primitives of every robot)
    and bases lie on the grid, from its initial state in the
    kernels' index arithmetic: how many corners and bases are outside the map, on which sides; how many have an integral grid
    coordinate; which cells of the bound table the bases index, the partial last row and column of cells among them."""
    field, root, dof, _ = scene(name)
    c = sole_corners(root, dof[:, :, 0]).astype(f32)
    p = ground_points(root, dof[:, :, 0]).astype(f32)
    out = {}
    for tag, (x, y) in (("corners", (c[:, :, 0].ravel(), c[:, :, 1].ravel())), ("points", (p[:, :, 0].ravel(), p[:, :, 1].ravel())),
                        ("bases", (root[:, 0], root[:, 1]))):
        u, v = field.uv(x, y)
        umax, vmax = f32(field.tot_rows - 1) - f32(1e-3), f32(field.tot_cols - 1) - f32(1e-3)
        out[tag] = dict(below_u=int((u < 0).sum()), above_u=int((u > umax).sum()), below_v=int((v < 0).sum()), above_v=int((v > vmax).sum()),
                        integral_u=int((u == np.floor(u)).sum()), integral_v=int((v == np.floor(v)).sum()),
                        near_u=int((np.abs(u - np.rint(u)) < 2e-5).sum()), near_v=int((np.abs(v - np.rint(v)) < 2e-5).sum()),
                        last_cell_u=int(((u > f32(field.tot_rows - 2)) & (u <= umax)).sum()), last_cell_v=int(((v > f32(field.tot_cols - 2)) & (v <= vmax)).sum()))
    cell = cell_samples(field.hscale)
    u, v = field.clamped(*field.uv(root[:, 0], root[:, 1]))
    out["cells"] = set(zip((u.astype(np.int32) // cell).tolist(), (v.astype(np.int32) // cell).tolist()))
    out["cell"], out["table"] = cell, (-(-field.tot_rows // cell), -(-field.tot_cols // cell))
    out["partial"] = (field.tot_rows % cell, field.tot_cols % cell)
    return out
