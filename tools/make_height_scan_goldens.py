"""Mints tests/golden/height_scan_ref.npz: what the REFERENCE's own height scan gives on seeded inputs.

Needs the reference checkout (oracle/ref_harness.py's DW_REFERENCE); nothing of it is copied.  Its isaacgym/torch_utils.py is imported from
where it lies; tasks/anymal_terrain.py cannot be imported (it pulls isaacgym.terrain_utils and the Gym bindings in), so the three functions
this needs -- init_height_points and get_heights of its task class and the module's quat_apply_yaw -- are cut out of the file's syntax tree
at run time and compiled as they stand, then called unbound on a stub `self`, on CPU torch.  The file written holds data only:

    grid [140, 2]                  x and y of init_height_points (env 0's rows; every env has the same)
    field_rough [70, 90], field_stairs [33, 27], field_tiny [2, 2]     int16 height samples
    vscale, obs_offset, obs_clip, obs_scale                            scalars (0.005; 0.5, 1, 5: the reference's line 302 and its yaml's scale)
    case_field [C], case_border [C], case_hscale [C]                   the twelve cases: field (0 rough, 1 stairs, 2 tiny) x border {0, 2} x hscale {0.1, 0.25}
    root [C, E, 13] float32        seeded root rows: yaw over the whole circle, tilt up to 1 rad about a horizontal axis, x and y over the
                                   whole map and up to 2 m outside it on all four sides, z in 0.3 .. 1.6
    heights [C, E, 140], obs [C, E, 140]     the reference's get_heights and clip(root_z - 0.5 - heights, -1, 1) * scale, float32
    d_u                            the largest deviation from float64 of a float32 evaluation of the header's steps 1 to 4 (grid coordinates)
    near [C, E, 140] bool          the point is near a line: either float64 grid coordinate is within 4 d_u of an integer

The inputs are drawn so that at most 2 % of the points are near a line (asserted; the share is printed): where a coordinate falls that
close to a sample line, which cell the reference reads is decided by its own rounding.  Two envs are near lines on purpose: env 0 of each of
the two rough cases at hscale 0.1 has yaw exactly 0 and its base on sample lines 31 and 47, so that all its 140 points (offsets of whole
tenths of a metre) have coordinates within an ulp of an integer: 280 points, 1.04 %.  With yaw 0 the rotation is exact, so there the
reference's cell is decided by its addition and its division alone -- these are the points that tell how it divides.  Minting twice
gives the same bytes (fixed seeds, fixed member dates)."""
import ast
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "height_scan_ref.npz")
E, VSCALE, OBS = 16, 0.005, (0.5, 1.0, 5.0)
PLACED = (31, 47)          # the sample lines the placed envs stand on
F = np.float32


def reference_functions():
    np.float = float          # (python/isaacgym/torch_utils.py:135 default argument, as oracle/ref_harness.py sets it)
    tu = ref_harness._load("dw_ref_torch_utils", os.path.join(ref_harness.PY, "isaacgym", "torch_utils.py"))
    path = os.path.join(ref_harness.IGE, "tasks", "anymal_terrain.py")
    tree = ast.parse(open(path).read(), path)
    want, found = {"init_height_points", "get_heights", "quat_apply_yaw"}, []
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in want:
            node.decorator_list = []          # (torch.jit.script needs the source file; eager gives the same numbers)
            found.append(node)
    assert {n.name for n in found} == want, [n.name for n in found]
    ns = {"torch": torch, "np": np, "normalize": tu.normalize, "quat_apply": tu.quat_apply}
    exec(compile(ast.Module(body=found, type_ignores=[]), path, "exec"), ns)
    return ns


class Stub:
    pass


def fields():
    rng = np.random.default_rng(3001)
    rough = rng.integers(-8, 9, size=(70, 90)).astype(np.int16)          # +-40 mm at 5 mm per unit
    i, j = np.meshgrid(np.arange(33), np.arange(27), indexing="ij")
    stairs = (12 * (i // 3) - 7 * (j // 4)).astype(np.int16)             # steps of 60 mm up along x every 3 samples, 35 mm down along y every 4
    tiny = np.array([[3, -2], [-5, 7]], np.int16)
    return [rough, stairs, tiny]


def roots(rng, rows, cols, hscale, border):
    x0, x1, y0, y1 = -border, (rows - 1) * hscale - border, -border, (cols - 1) * hscale - border
    r = np.zeros((E, 13))
    r[:, 0], r[:, 1] = rng.uniform(x0 - 2, x1 + 2, E), rng.uniform(y0 - 2, y1 + 2, E)
    r[:, 2] = rng.uniform(0.3, 1.6, E)
    yaw, tilt, ax = rng.uniform(-np.pi, np.pi, E), rng.uniform(0, 1.0, E), rng.uniform(-np.pi, np.pi, E)
    qy = np.stack([0 * yaw, 0 * yaw, np.sin(yaw / 2), np.cos(yaw / 2)], 1)
    qt = np.stack([np.cos(ax) * np.sin(tilt / 2), np.sin(ax) * np.sin(tilt / 2), 0 * ax, np.cos(tilt / 2)], 1)
    x1_, y1_, z1_, w1_ = qy.T
    x2_, y2_, z2_, w2_ = qt.T
    r[:, 3:7] = np.stack([w1_ * x2_ + x1_ * w2_ + y1_ * z2_ - z1_ * y2_, w1_ * y2_ - x1_ * z2_ + y1_ * w2_ + z1_ * x2_,
                          w1_ * z2_ + x1_ * y2_ - y1_ * x2_ + z1_ * w2_, w1_ * w2_ - x1_ * x2_ - y1_ * y2_ - z1_ * z2_], 1)
    r[:, 7:13] = rng.normal(size=(E, 6)) * 0.3
    return r.astype(F)


def coordinates(root, grid, border, hscale, dt):
    """The grid coordinates (u, v) [E, P] of the header's steps 1 to 4 (gpu_div = 0) in dtype dt, every operation rounded in dt."""
    r, g, b, h = root.astype(dt), grid.astype(dt), dt(F(border)), dt(F(hscale))          # (the scales are float32 numbers in either)
    qz, qw = r[:, 5:6], r[:, 6:7]
    n = np.maximum(np.sqrt(qz * qz + qw * qw), dt(1e-9))
    z, w = qz / n, qw / n
    ox, oy = g[None, :, 0], g[None, :, 1]
    tx, ty = -(z * oy) * dt(2), (z * ox) * dt(2)
    X, Y = (ox + w * tx) - z * ty, (oy + w * ty) + z * tx
    return ((X + r[:, 0:1]) + b) / h, ((Y + r[:, 1:2]) + b) / h


def compute():
    ns = reference_functions()
    hs = fields()
    s = Stub()
    s.device, s.num_envs = "cpu", E
    pts = ns["init_height_points"](s)
    s.num_height_points, s.height_points = pts.shape[1], pts
    grid = pts[0, :, :2].numpy().copy()
    assert grid.shape == (140, 2) and (pts[:, :, :2] == pts[0:1, :, :2]).all() and (pts[:, :, 2] == 0).all()
    s.cfg = {"env": {"terrain": {"terrainType": "trimesh"}}}
    rng = np.random.default_rng(3002)
    cases = [(f, b, h) for f in range(3) for b in (0.0, 2.0) for h in (0.1, 0.25)]
    root, heights, obs, u64, v64, du = [], [], [], [], [], 0.0
    for f, b, h in cases:
        r = roots(rng, hs[f].shape[0], hs[f].shape[1], h, b)
        if f == 0 and h == 0.1:          # one env of each rough 0.1 m case stands ON sample lines, heading along x (see the docstring)
            r[0, 0], r[0, 1], r[0, 3:7] = F(PLACED[0] * h - b), F(PLACED[1] * h - b), (0, 0, 0, 1)
        s.root_states = torch.from_numpy(r.copy())
        s.base_quat = s.root_states[:, 3:7]
        s.height_samples = torch.from_numpy(hs[f].copy())
        s.terrain = Stub()
        s.terrain.border_size, s.terrain.horizontal_scale, s.terrain.vertical_scale = b, h, VSCALE
        ht = ns["get_heights"](s)
        assert ht.dtype == torch.float32 and ht.shape == (E, 140)
        ob = torch.clip(s.root_states[:, 2].unsqueeze(1) - OBS[0] - ht, -OBS[1], OBS[1]) * OBS[2]
        root.append(r); heights.append(ht.numpy().copy()); obs.append(ob.numpy().copy())
        a64, c64 = coordinates(r, grid, b, h, np.float64)
        a32, c32 = coordinates(r, grid, b, h, np.float32)
        du = max(du, float(np.abs(a32.astype(np.float64) - a64).max()), float(np.abs(c32.astype(np.float64) - c64).max()))
        u64.append(a64); v64.append(c64)
    u64, v64 = np.stack(u64), np.stack(v64)
    near = (np.abs(u64 - np.rint(u64)) <= 4 * du) | (np.abs(v64 - np.rint(v64)) <= 4 * du)
    share = float(near.mean())
    print("d_u = %.3e grid units; near a line: %d of %d points (%.3f %%)" % (du, near.sum(), near.size, 100 * share))
    assert share <= 0.02, share
    return dict(grid=grid, field_rough=hs[0], field_stairs=hs[1], field_tiny=hs[2], vscale=F(VSCALE), obs_offset=F(OBS[0]), obs_clip=F(OBS[1]),
                obs_scale=F(OBS[2]), case_field=np.array([c[0] for c in cases], np.int32), case_border=np.array([c[1] for c in cases], F),
                case_hscale=np.array([c[2] for c in cases], F), root=np.stack(root), heights=np.stack(heights), obs=np.stack(obs),
                d_u=np.float64(du), near=near)


def save(path: str, arrays: dict):
    """np.savez_compressed's format with fixed member dates and order, so the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, np.asarray(arrays[k], order="C"), allow_pickle=False)          # (asarray: a scalar stays 0-d)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


if __name__ == "__main__":
    save(OUT, compute())
    print(OUT, os.path.getsize(OUT))
