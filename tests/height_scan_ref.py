"""Test helper of the terrain height scan (include/dyros_height_scan.h).  Four parts:

  (a) scan32: a numpy float32 restatement of the header, operation for operation (every intermediate a float32 array, no fused
      multiply-add): the grid by either rule and either gpu_div, the observation line, the probes by dw_bodies.h's chain and
      dw_physics.h's terrain_sample.  `bug` injects the mistakes the fixture check must reject.
  (b) truth64: float64 truth for the grid points, the bilinear rule and the probes, from terrain_edge_cases.Field.height_at and fk.
  (c) torch_twin: the reference's lines (quat_apply_yaw, quat_apply, get_heights) written in eager torch, for the comparison on the GPU
      and as "today's path" of tools/height_scan_time.py.
  (d) channel_d: per channel, d = the largest deviation of (a) from (b) over 4096 seeded cases on the field under test.  It is never
      measured against a kernel or the g++ build; what is tested is held within 4 d (the project's rule, tests/terrain_edge_cases.py).

Near a line: a point either of whose float64 grid coordinates lies within 4 d_u of an integer, d_u = the largest deviation of (a)'s float32
coordinate from the float64 one on the same inputs.  There the cell a float32 evaluation lands in is decided by its own rounding: the
nearest rule's height and the ground's normal are held only away from lines, and at most 2 % of a test's points may be near one."""
import numpy as np

import terrain_edge_cases as TE
from isaacgymdyros_amd import body_states as BS
from isaacgymdyros_amd import height_scan as H

F = np.float32
K = H.K
BUGS = ("rows_for_cols", "straight_neighbour", "max_for_min", "full_quaternion", "unrotated", "clip_rows_minus_1", "multiply_under_cpu_div")
NEAR_CAP = 0.02
T_MV, T_CARRIER = BS.K["DWB_T_MV"], BS.K["DWB_T_CARRIER"]


# ---------------------------------------------------------------------------------------------- (a) float32, operation for operation
def yaw_pair32(root):
    qz, qw = root[:, 5], root[:, 6]
    n = np.maximum(np.sqrt(qz * qz + qw * qw), F(1e-9))
    return qz / n, qw / n


def grid_points32(root, grid, bug=None):
    """(xw, yw) [N, P] of steps 1 to 3."""
    root, grid = np.asarray(root, F), np.asarray(grid, F)
    ox, oy = grid[None, :, 0], grid[None, :, 1]
    if bug == "unrotated":
        return ox + root[:, 0:1], oy + root[:, 1:2]
    if bug == "full_quaternion":
        q = root[:, 3:7] / np.sqrt(((root[:, 3] * root[:, 3] + root[:, 4] * root[:, 4]) + root[:, 5] * root[:, 5]) + root[:, 6] * root[:, 6])[:, None]
        x, y, z, w = (q[:, i:i + 1] for i in range(4))
        tx, ty, tz = (-(z * oy)) * F(2), (z * ox) * F(2), (x * oy - y * ox) * F(2)
        return (ox + w * tx) + (y * tz - z * ty) + root[:, 0:1], (oy + w * ty) + (z * tx - x * tz) + root[:, 1:2]
    z, w = (a[:, None] for a in yaw_pair32(root))
    tx, ty = -(z * oy) * F(2), (z * ox) * F(2)
    X, Y = (ox + w * tx) - z * ty, (oy + w * ty) + z * tx
    return X + root[:, 0:1], Y + root[:, 1:2]


def coord32(x, border, hscale, gpu_div):
    return (x + F(border)) * (F(1.0) / F(hscale)) if gpu_div else (x + F(border)) / F(hscale)


def cell32(u, n):
    hi = F(n - 2)
    with np.errstate(invalid="ignore"):
        return np.where(u > 0, np.where(u > hi, hi, u), F(0)).astype(np.int32)


def sample32(hs, hscale, vscale, border, x, y, normal=False):
    """dw_physics.h terrain_sample in float32: the bilinear height (and the unit normal, host form: 1 / sqrtf) under world points."""
    hs = np.asarray(hs)
    rows, cols = hs.shape
    inv, vs = F(1.0) / F(hscale), F(vscale)
    u, v = (x + F(border)) * inv, (y + F(border)) * inv
    umax, vmax = F(rows - 1) - F(1e-3), F(cols - 1) - F(1e-3)
    with np.errstate(invalid="ignore"):
        u = np.where(u > 0, np.where(u > umax, umax, u), F(0))
        v = np.where(v > 0, np.where(v > vmax, vmax, v), F(0))
    i, j = u.astype(np.int32), v.astype(np.int32)
    a, b = u - i.astype(F), v - j.astype(F)
    h00, h01, h10, h11 = hs[i, j].astype(F), hs[i, j + 1].astype(F), hs[i + 1, j].astype(F), hs[i + 1, j + 1].astype(F)
    one = F(1.0)
    h = vs * ((one - a) * ((one - b) * h00 + b * h01) + a * ((one - b) * h10 + b * h11))
    if not normal:
        return h
    gx = vs * inv * ((one - b) * (h10 - h00) + b * (h11 - h01))
    gy = vs * inv * ((one - a) * (h01 - h00) + a * (h11 - h10))
    nn = one / np.sqrt(gx * gx + gy * gy + one)
    return h, np.stack([-gx * nn, -gy * nn, nn], -1)


def grid32(root, grid, hs, hscale=0.1, vscale=0.005, border=0.0, rule="nearest", gpu_div=0, obs=None, bug=None):
    """dict(points [N, P, 2], heights [N, P], obs [N, P] or None) of the header in float32.  hs None: the plane."""
    root = np.asarray(root, F)
    xw, yw = grid_points32(root, grid, bug)
    if hs is None:
        h = np.zeros(xw.shape, F)
    elif rule == "bilinear":
        h = sample32(hs, hscale, vscale, border, xw, yw)
    else:
        hs = np.asarray(hs)
        rows, cols = hs.shape[::-1] if bug == "rows_for_cols" else hs.shape
        flat = hs.reshape(rows, cols)          # (rows taken for cols: the same samples in memory read with the other pitch)
        div = 1 if bug == "multiply_under_cpu_div" else gpu_div
        cut = 1 if bug == "clip_rows_minus_1" else 0
        i, j = cell32(coord32(xw, border, hscale, div), rows + cut), cell32(coord32(yw, border, hscale, div), cols + cut)
        i2, j2 = np.minimum(i + 1, rows - 1), (j if bug == "straight_neighbour" else np.minimum(j + 1, cols - 1))
        pick = np.maximum if bug == "max_for_min" else np.minimum
        h = pick(flat[i, j], flat[i2, j2]).astype(F) * F(vscale)
    out = dict(points=np.stack([xw, yw], -1), heights=h, obs=None)
    if obs is not None:
        off, c, s = (F(x) for x in obs)
        out["obs"] = np.clip((root[:, 2:3] - off) - h, -c, c) * s
    return out


def _quat_mul32(a, b):
    return np.stack([a[:, 3] * b[:, 0] + a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 3] * b[:, 1] - a[:, 0] * b[:, 2] + a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0],
                     a[:, 3] * b[:, 2] + a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3],
                     a[:, 3] * b[:, 3] - a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2]], 1)


def _quat_to_mat32(q):
    X, Y, Z, W = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = F(1), F(2)
    return np.stack([one - two * (Y * Y + Z * Z), two * (X * Y - W * Z), two * (X * Z + W * Y), two * (X * Y + W * Z), one - two * (X * X + Z * Z),
                     two * (Y * Z - W * X), two * (X * Z - W * Y), two * (Y * Z + W * X), one - two * (X * X + Y * Y)], 1)


def _m3v32(R, v):
    return np.stack([R[:, 3 * i] * v[..., 0] + R[:, 3 * i + 1] * v[..., 1] + R[:, 3 * i + 2] * v[..., 2] for i in range(3)], 1)


def carrier_pose32(table, m, root, dof):
    """(off [N, 3], R [N, 9]) of moving body m by dw_bodies.h's base() and child() in float32; table: a packed table's words."""
    mv = table[T_MV:T_MV + 34 * 11].reshape(34, 11)
    parent = mv[:, 0].view(np.int32)
    c = mv.view(F)
    chain = []
    while m > 0:
        chain.insert(0, int(m))
        m = parent[m]
    root, dof = np.asarray(root, F), np.asarray(dof, F).reshape(len(root), 33, 2)
    n = np.sqrt(root[:, 3] * root[:, 3] + root[:, 4] * root[:, 4] + root[:, 5] * root[:, 5] + root[:, 6] * root[:, 6])
    q = root[:, 3:7] / n[:, None]
    R, off = _quat_to_mat32(q), np.zeros((len(root), 3), F)
    for b in chain:
        pos, q0, ax = c[b, 1:4], c[b, 4:8], c[b, 8:11]
        off = off + _m3v32(R, pos)
        h = F(0.5) * dof[:, b - 1, 0]
        sn, cs = np.sin(h), np.cos(h)
        qj = np.stack([ax[0] * sn, ax[1] * sn, ax[2] * sn, cs], 1)
        q = _quat_mul32(q, _quat_mul32(np.broadcast_to(q0, qj.shape), qj))
        R = _quat_to_mat32(q)
    return off, R


def probes32(table, probes, root, dof, hs, hscale=0.1, vscale=0.005, border=0.0):
    """dict(probe_pos [N, B, 3], probe_height, clearance [N, B], probe_normal [N, B, 3]) of the header in float32; probes: resolved dicts."""
    root = np.asarray(root, F)
    carrier = table[T_CARRIER:T_CARRIER + 38].view(np.int32)
    pos = []
    for p in probes:
        off, R = carrier_pose32(table, carrier[p["gym"]], root, dof)
        pos.append(root[:, :3] + (off + _m3v32(R, np.asarray(p["pos"], F))))
    pos = np.stack(pos, 1)
    if hs is None:
        h, n = np.zeros(pos.shape[:2], F), np.broadcast_to(np.array([0, 0, 1], F), pos.shape).copy()
        return dict(probe_pos=pos, probe_height=h, clearance=pos[..., 2].copy(), probe_normal=n)
    h, n = sample32(hs, hscale, vscale, border, pos[..., 0], pos[..., 1], normal=True)
    return dict(probe_pos=pos, probe_height=h, clearance=pos[..., 2] - h, probe_normal=n)


# ---------------------------------------------------------------------------------------------- (b) float64 truth
def grid_points64(root, grid):
    r, g = np.asarray(root, np.float64), np.asarray(grid, np.float64)
    n = np.maximum(np.hypot(r[:, 5], r[:, 6]), 1e-9)
    z, w = (r[:, 5] / n)[:, None], (r[:, 6] / n)[:, None]
    ox, oy = g[None, :, 0], g[None, :, 1]
    c, s = w * w - z * z, 2 * z * w          # cos and sin of the yaw
    return c * ox - s * oy + r[:, 0:1], s * ox + c * oy + r[:, 1:2]


def coords64(root, grid, border, hscale):
    x, y = grid_points64(root, grid)
    return (x + float(F(border))) / float(F(hscale)), (y + float(F(border))) / float(F(hscale))


def normal64(field, x, y):
    u = np.clip((x + field.border) / field.hscale, 0.0, field.tot_rows - 1 - 1e-3)
    v = np.clip((y + field.border) / field.hscale, 0.0, field.tot_cols - 1 - 1e-3)
    i, j = u.astype(int), v.astype(int)
    a, b = u - i, v - j
    h = field.heightsamples.astype(np.float64)
    k = field.vscale / field.hscale
    gx = k * ((1 - b) * (h[i + 1, j] - h[i, j]) + b * (h[i + 1, j + 1] - h[i, j + 1]))
    gy = k * ((1 - a) * (h[i, j + 1] - h[i, j]) + a * (h[i + 1, j + 1] - h[i + 1, j]))
    nn = 1.0 / np.sqrt(gx * gx + gy * gy + 1.0)
    return np.stack([-gx * nn, -gy * nn, nn], -1)


def truth64(field, root, dof, grid, probes):
    """Float64: dict(points, bilinear [N, P], probe_pos, probe_height, clearance, probe_normal) from Field.height_at and fk."""
    x, y = grid_points64(root, grid)
    out = dict(points=np.stack([x, y], -1), bilinear=field.height_at(x, y))
    if probes:
        q = np.asarray(dof, np.float64).reshape(len(root), 33, 2)[:, :, 0]
        xb, Rb = TE.fk(root, q)
        mv = np.asarray(TE.MODEL.body_moving)
        pos = np.stack([xb[:, mv[p["gym"]]] + Rb[:, mv[p["gym"]]] @ np.asarray(p["pos"], np.float64) for p in probes], 1)
        h = field.height_at(pos[..., 0], pos[..., 1])
        out.update(probe_pos=pos, probe_height=h, clearance=pos[..., 2] - h, probe_normal=normal64(field, pos[..., 0], pos[..., 1]))
    return out


def near_line(u64, v64, d_u):
    return (np.abs(u64 - np.rint(u64)) <= 4 * d_u) | (np.abs(v64 - np.rint(v64)) <= 4 * d_u)


def d_u_of(root, grid, border, hscale, gpu_div=0):
    """The largest deviation of (a)'s float32 grid coordinates from the float64 ones on these inputs."""
    xw, yw = grid_points32(root, grid)
    u64, v64 = coords64(root, grid, border, hscale)
    u, v = coord32(xw, border, hscale, gpu_div), coord32(yw, border, hscale, gpu_div)
    return float(max(np.abs(u.astype(np.float64) - u64).max(), np.abs(v.astype(np.float64) - v64).max()))


# ---------------------------------------------------------------------------------------------- (c) the reference's lines in torch
def torch_twin(root, points3, hs, border, hscale, vscale):
    """The reference's get_heights on torch tensors of any device: root [N, 13], points3 [N, P, 3] (z zero), hs int16 [rows, cols]."""
    import torch
    N, P = points3.shape[:2]
    q = root[:, 3:7].clone().view(-1, 4)
    q[:, :2] = 0.0
    q = q / q.norm(p=2, dim=-1).clamp(min=1e-9, max=None).unsqueeze(-1)
    a, b = q.repeat(1, P).reshape(-1, 4), points3.reshape(-1, 3)
    xyz = a[:, :3]
    t = xyz.cross(b, dim=-1) * 2
    pts = (b + a[:, 3:] * t + xyz.cross(t, dim=-1)).view(N, P, 3) + root[:, :3].unsqueeze(1)
    pts += border
    pts = (pts / hscale).long()
    px = torch.clip(pts[:, :, 0].view(-1), 0, hs.shape[0] - 2)
    py = torch.clip(pts[:, :, 1].view(-1), 0, hs.shape[1] - 2)
    return torch.min(hs[px, py], hs[px + 1, py + 1]).view(N, -1) * vscale


# ---------------------------------------------------------------------------------------------- (d) the per-channel d
CASES = 4096
_d = {}


def seeded_cases(field, seed=4201, n=CASES):
    """Roots and joint rows over the whole map and 0.5 m outside it: yaw over the circle, tilt up to 0.3 rad, near the ground."""
    rng = np.random.default_rng(seed)
    (x0, x1), (y0, y1) = field.extent
    root = np.zeros((n, 13))
    root[:, 0], root[:, 1] = rng.uniform(x0 - 0.5, x1 + 0.5, n), rng.uniform(y0 - 0.5, y1 + 0.5, n)
    root[:, 3:7] = TE._yaw_quat(rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.3, 0.3, (n, 2)))
    root[:, 2] = field.height_at(root[:, 0], root[:, 1]) + rng.uniform(0.85, 1.0, n)
    dof = np.zeros((n, 33, 2))
    dof[:, :, 0] = TE.Q0 + rng.normal(size=(n, 33)) * 0.1
    return root.astype(F), dof.astype(F)


def channel_d(field, table, grid, probes, key):
    """d per channel for this field (cached under key): bilinear, probe_pos, probe_height, clearance, probe_normal (the last away from lines)."""
    if key not in _d:
        root, dof = seeded_cases(field)
        args = (field.heightsamples, field.hscale, field.vscale, field.border)
        a = grid32(root, grid, *args, rule="bilinear")
        a.update(probes32(table, probes, root, dof, *args))
        b = truth64(field, root, dof, grid, probes)
        d = dict(bilinear=float(np.abs(a["heights"] - b["bilinear"]).max()), points=float(np.abs(a["points"] - b["points"]).max()))
        for k in ("probe_pos", "probe_height", "clearance"):
            d[k] = float(np.abs(a[k] - b[k]).max())
        away = ~probe_near(field, b["probe_pos"], a["probe_pos"])
        d["probe_normal"] = float(np.abs(a["probe_normal"] - b["probe_normal"])[away].max())
        _d[key] = d
    return _d[key]


def probe_near(field, pos64, pos32):
    """Probes near a line: the band is 4 x the largest deviation of the float32 grid coordinate of pos32 from the float64 one of pos64."""
    u64, v64 = (pos64[..., 0] + field.border) / field.hscale, (pos64[..., 1] + field.border) / field.hscale
    u32, v32 = TE.Field.uv(field, pos32[..., 0], pos32[..., 1])
    du = float(max(np.abs(u32 - u64).max(), np.abs(v32 - v64).max()))
    return near_line(u64, v64, du)
