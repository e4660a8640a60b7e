"""The terrain height scan (include/dyros_height_scan.h, csrc/dw_height_scan.hip): the reference's init_height_points /
get_heights (tasks/anymal_terrain.py:501-536) -- the ground's heights at a yaw-aligned grid of points around the base -- and the clearance
over the ground of points fixed to bodies, by default the eight sole corners the contact solve samples.

Opt-in: cfg["sim"]["mi355"]["height_scan"] = True, or {"grid": {"x": [...], "y": [...]} or a list of [x, y], "rule": "nearest" | "bilinear",
"probes": "soles" | [{"body", "pos"}] | None, "normals": False, "points": False, "obs": None | {"offset": 0.5, "clip": 1.0, "scale": 1.0},
"auto": False}, gives a DyrosDynamicWalk env a `height_scan` attribute (None otherwise; TocabiAMPLower: key `amp_height_scan`).  refresh()
makes one launch, dwh_scan, on torch's current stream, from the bound root_states, dof_state and height_samples (the plane where the env has
no height field: zeros, and the probes' clearance is their z).  It only reads the env's buffers, takes no argument that changes from call to
call, allocates nothing and does not synchronise, so it sits inside a captured rollout step.

    refresh()                 one launch; returns `heights` [N, P]   (= env.get_heights())
    heights                   [N, P]: rule "nearest" = the reference's get_heights, "bilinear" = the height the contact solve sees there
    points                    [N, P, 2]: the grid points' world x, y (None unless "points": True)
    obs                       [N, P]: clip(root_z - offset - heights, -clip, clip) * scale, the reference's line 302 (None unless "obs")
    probe_pos, probe_heights, clearance      [N, B, 3], [N, B], [N, B]: the probes' world positions, the bilinear height under them, z - height
    probe_normals             [N, B, 3]: the ground's unit normal under the probes (None unless "normals": True)
    grid, names               [P, 2] float32 offsets in the base's yaw frame (x-major for a {"x", "y"} grid); the probes' body names

"auto": True refreshes after every step(), after reset_idx() and reset().  The contact solve's depth of a sole corner is
clearance * probe_normals[..., 2] (section 30).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import cbind
from .model_tensors import ModelTensor, ptr, resolve_front

K = cbind.constants("dyros_height_scan.h", "dwh_")
EXPORTS = list(cbind.signatures("dyros_height_scan.h", "dwh_"))
_S = cbind.structs("dyros_height_scan.h", "dwh_")
DwhProbe, DwhParams = _S["DwhProbe"], _S["DwhParams"]
MAX_POINTS, MAX_PROBES, GROUP, TABLE_WORDS = K["DWH_MAX_POINTS"], K["DWH_MAX_PROBES"], K["DWH_GROUP"], K["DWH_TABLE_WORDS"]
MAX_SIDE = 8192          # samples along a side of the map (include/dyros_height_scan.h)
RULES = {"nearest": K["DWH_RULE_NEAREST"], "bilinear": K["DWH_RULE_BILINEAR"]}
# the reference's init_height_points, in tenths of a metre
GRID_X, GRID_Y = (-8, -7, -6, -5, -4, -3, -2, 2, 3, 4, 5, 6, 7, 8), (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)
DEFAULTS = {"grid": None, "rule": "nearest", "probes": "soles", "normals": False, "points": False, "obs": None, "auto": False}
OBS_DEFAULTS = {"offset": 0.5, "clip": 1.0, "scale": 1.0}


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_height_scan.h", "dwh_")


def default_grid() -> np.ndarray:
    """[140, 2] float32: x = 0.1 * GRID_X and y = 0.1 * GRID_Y, each product rounded to float32 as the reference's tensors are, x-major."""
    x, y = np.float32(0.1) * np.asarray(GRID_X, np.float32), np.float32(0.1) * np.asarray(GRID_Y, np.float32)
    return mesh(x, y)


def mesh(x, y) -> np.ndarray:
    """meshgrid(x, y) flattened x-major: [len(x) * len(y), 2]."""
    x, y = np.asarray(x, np.float32).ravel(), np.asarray(y, np.float32).ravel()
    return np.stack([np.repeat(x, len(y)), np.tile(y, len(x))], 1).astype(np.float32)


def _floats(what, v, n=None):
    try:
        a = [float(x) for x in v]
    except (TypeError, ValueError):
        a = None
    if a is None or isinstance(v, (str, bytes)) or (n is not None and len(a) != n) or not all(math.isfinite(x) for x in a):
        raise ValueError("height_scan: %s must be %s finite numbers" % (what, "a list of" if n is None else n))
    return a


def _grid(g) -> np.ndarray:
    if g is None:
        return default_grid()
    if isinstance(g, dict):
        if set(g) != {"x", "y"}:
            raise ValueError("height_scan.grid: a dict holds x and y, the two axes of a meshgrid")
        out = mesh(_floats("grid.x", g["x"]), _floats("grid.y", g["y"]))
    else:
        if isinstance(g, (str, bytes)) or not hasattr(g, "__len__"):
            raise ValueError("height_scan.grid must be {'x': [...], 'y': [...]} or a list of [x, y] offsets")
        out = np.asarray([_floats("a grid point", p, 2) for p in g], np.float32).reshape(-1, 2)
    if not 1 <= len(out) <= MAX_POINTS:
        raise ValueError("height_scan.grid must hold 1..%d points, got %d" % (MAX_POINTS, len(out)))
    if not np.isfinite(out).all():
        raise ValueError("height_scan.grid: an offset is not finite in float32")
    return out


def _probes(p, model) -> list:
    if p is None:
        return []
    if isinstance(p, str):
        if p != "soles":
            raise ValueError("height_scan.probes must be 'soles', None or a list of {'body', 'pos'} dicts")
        names = list(model.body_names)
        return [{"body": names[f["gym"]], "gym": int(f["gym"]), "pos": [float(x) for x in f["pos"]]} for f in model.foot_pts]
    if isinstance(p, (bytes, dict)) or not hasattr(p, "__len__") or len(p) > MAX_PROBES:
        raise ValueError("height_scan.probes must be 'soles', None or a list of at most %d {'body', 'pos'} dicts" % MAX_PROBES)
    names, out = list(model.body_names), []
    for s in p:
        if not isinstance(s, dict) or set(s) - {"body", "pos"} or "body" not in s:
            raise ValueError("height_scan.probes: a probe is a dict with body and optionally pos; got %r" % (s,))
        b = s["body"]
        g = names.index(b) if isinstance(b, str) and b in names else (int(b) if isinstance(b, (int, np.integer)) and not isinstance(b, bool) else -1)
        if not 0 <= g < len(names):
            raise ValueError("height_scan.probes: %r is neither a body name nor a Gym id in 0..%d" % (b, len(names) - 1))
        out.append({"body": names[g], "gym": g, "pos": _floats("a probe's pos", s.get("pos", (0.0, 0.0, 0.0)), 3)})
    return out


def resolve(spec, model=None, terrain=None) -> dict:
    """The cfg value as a full dict; None when the scan is off (None or False).  ValueError for anything else that is not True or a dict of
    grid / rule / probes / normals / points / obs / auto, for a grid of no or too many points, an unknown rule, a probe on an unknown body,
    an obs that is not a dict of offset / clip / scale, and for terrain: a height-field cfg["terrain"] whose scales are not positive.
    model: a TocabiModel (None: the packaged one).  In the result grid is [P, 2] float32, rule the header's number, probes full dicts."""
    out = resolve_front("height_scan", spec, DEFAULTS, ("normals", "points", "auto"), "grid, rule, probes, normals, points, obs and auto")
    if out is None:
        return None
    t = dict(terrain or {})
    if t.get("mesh_type", "plane") in ("heightfield", "trimesh"):
        for k in ("horizontal_scale", "vertical_scale"):
            if k in t and not (isinstance(t[k], (int, float)) and math.isfinite(t[k]) and t[k] > 0):
                raise ValueError("height_scan: terrain.%s must be finite and > 0" % k)
    if model is None:
        from .model import load_model
        model = load_model()
    if out["rule"] not in RULES:
        raise ValueError("height_scan.rule must be one of %s" % sorted(RULES))
    out["grid"], out["rule_id"] = _grid(out["grid"]), RULES[out["rule"]]
    out["probes"] = _probes(out["probes"], model)
    if out["normals"] and not out["probes"]:
        raise ValueError("height_scan.normals: there is no probe to give a normal for")
    if out["obs"] is not None:
        if out["obs"] is True:
            out["obs"] = {}
        if not isinstance(out["obs"], dict) or set(out["obs"]) - set(OBS_DEFAULTS):
            raise ValueError("height_scan.obs must be None or a dict of offset, clip and scale")
        o = dict(OBS_DEFAULTS, **out["obs"])
        o = dict(zip(OBS_DEFAULTS, _floats("obs.offset, obs.clip and obs.scale", [o[k] for k in OBS_DEFAULTS], 3)))
        if o["clip"] < 0:
            raise ValueError("height_scan.obs.clip must be >= 0")
        out["obs"] = o
    return out


def validate(spec, terrain=None) -> None:
    """Checks of cfg sim.mi355.height_scan (config.validate_cfg)."""
    resolve(spec, terrain=terrain)


def params_struct(rows=0, cols=0, hscale=1.0, vscale=1.0, border=0.0, obs=None) -> DwhParams:
    p, o = DwhParams(), dict(OBS_DEFAULTS, **(obs or {}))
    p.rows, p.cols, p.hscale, p.vscale, p.border = int(rows), int(cols), float(hscale), float(vscale), float(border)
    p.obs_offset, p.obs_clip, p.obs_scale = float(o["offset"]), float(o["clip"]), float(o["scale"])
    return p


def probe_array(probes):
    """(DwhProbe * B)() of resolved probe dicts (None for none)."""
    if not probes:
        return None
    arr = (DwhProbe * len(probes))()
    for a, s in zip(arr, probes):
        a.body = int(s["gym"])
        for i in range(3):
            a.pos[i] = s["pos"][i]
    return arr


def pack_table(api: dict, model, grid, probes, params) -> np.ndarray:
    """The device table's DWH_TABLE_WORDS words as a uint32 array (dwh_pack_table; raises for what it refuses).  model: a TocabiModel, its
    dictionary or a DwbModel; grid [P, 2]; probes: resolved dicts, a DwhProbe array or None; params: a DwhParams."""
    from .body_states import DwbModel, model_struct
    m = model if isinstance(model, DwbModel) else model_struct(model)
    g = np.ascontiguousarray(grid, np.float32).reshape(-1, 2)
    arr = probe_array(probes) if isinstance(probes, (list, tuple)) else probes
    t = np.zeros(TABLE_WORDS, np.uint32)
    cbind.check(api, api["pack_table"](C.byref(m), g.ctypes.data, len(g), arr, 0 if arr is None else len(arr), C.byref(params), t.ctypes.data))
    return t


class HeightScan(ModelTensor):
    """The height scan of one env object's bound buffers (see the module docstring).  host: a DyrosDynamicWalk (TocabiAMPLower hands its
    physics host).  Buffers are allocated here, once."""

    WHAT = "scan"

    def __init__(self, host, spec=True):
        import torch
        model = host.model
        spec = resolve(spec, model)
        super().__init__(host, spec, declare)
        N, c = self.num_envs, host._ccfg
        self.rule, self.grid = spec["rule"], spec["grid"]
        self.probes = spec["probes"]
        self.names = [p["body"] for p in self.probes]
        self.dt = float(host.dt) * int(getattr(host, "skipframe", 1))
        self.gpu_div = int(bool(c.torch_gpu_div))
        if getattr(host, "custom_origins", False):
            hs = host._buf["height_samples"]
            rows, cols = int(c.terrain_rows), int(c.terrain_cols)
            if hs.dtype != torch.int16 or hs.numel() != rows * cols or not hs.is_contiguous():
                raise ValueError("height_scan: height_samples must be %d x %d contiguous int16" % (rows, cols))
            if max(rows, cols) > MAX_SIDE:
                raise ValueError("height_scan: a map side must not exceed %d samples, the map is %d x %d" % (MAX_SIDE, rows, cols))
            self._map = (hs.data_ptr(), rows, cols, float(c.terrain_hscale), float(c.terrain_vscale), float(c.terrain_border))
        else:
            self._map = (None, 0, 0, 1.0, 1.0, 0.0)
        self.params = params_struct(*self._map[1:], obs=spec["obs"])
        self.table = self._upload(pack_table(self.api, model, self.grid, self.probes, self.params))
        P, B = len(self.grid), len(self.probes)
        self.heights = self._zeros(N, P)
        self.points = self._zeros(N, P, 2) if spec["points"] else None
        self.obs = self._zeros(N, P) if spec["obs"] is not None else None
        self.probe_pos = self._zeros(N, B, 3) if B else None
        self.probe_heights = self._zeros(N, B) if B else None
        self.clearance = self._zeros(N, B) if B else None
        self.probe_normals = self._zeros(N, B, 3) if spec["normals"] else None
        self._args = self._inputs() + self._map + (spec["rule_id"], self.gpu_div, ptr(self.heights), ptr(self.points), ptr(self.obs),
                                                   ptr(self.probe_pos), ptr(self.probe_heights), ptr(self.clearance), ptr(self.probe_normals))

    def refresh(self):
        """One launch on torch's current stream; returns `heights`."""
        self._launch("scan", self._args)
        return self.heights

    def index(self, name: str) -> int:
        """The first probe on a body."""
        if name not in self.names:
            raise KeyError("height_scan holds no probe on %r" % (name,))
        return self.names.index(name)
