"""The inverse kinematics (include/dyros_inverse_kinematics.h, csrc/dw_inverse_kinematics.hip): the joint angles -- and,
when asked, the base pose -- that put chosen bodies at wanted poses, in the coordinates of isaacgymdyros_amd/jacobians.py.  Every other model
tensor answers a question about the state the simulator is in; this one asks which state puts a foot or a hand where the caller wants it:
to stand a batch of robots with both soles on the ground, to retarget a motion to other link lengths, to hand contact_inverse_dynamics a
posture to hold, to place a foot.  One launch runs up to "iterations" damped-least-squares steps per env, dnu = J' (J J' + lambda^2 W^-1)^-1 e,
with the chain walk, J, the factor and the update all in the env's LDS; an env that meets the tolerances stops moving.

Opt-in: cfg["sim"]["mi355"]["inverse_kinematics"] = True, or {"targets": [{"body": "L_Foot_Link", "pos": [0, 0, -0.09]}, {"body":
"R_Foot_Link", "pos": [0, 0, -0.09]}], "rows": None, "weights": None, "dofs": None, "base": False, "iterations": 16, "damping": 0.05,
"max_step": 0.5, "tol_pos": 1e-5, "tol_ang": 1e-5, "limits": True, "target_frame": "world", "auto": False}, gives a DyrosDynamicWalk env an
`inverse_kinematics` attribute (None otherwise; TocabiAMPLower: key `amp_inverse_kinematics`).  Each call only reads the env's buffers, takes
no argument that changes from call to call, allocates nothing and does not synchronise, so it sits inside a captured rollout step.

Targets are contact_dynamics.py's contacts: a Gym body (name or id) and a point `pos` in its frame; 1 .. 4 targets, no two on one moving
body; six rows each (the point's position, the body's orientation, world axes), m = 6 K.  "rows": per target "pose", "position" or
"orientation" (None: poses).  "weights": None (ones), six positive numbers (every target's) or K lists of six: a larger weight makes a row's
error dearer against the damping.  "dofs": the joints that may move, names or Gym DoF ids (None: the joints on the paths from the base to the
targets' bodies -- 12 for both feet); every other joint keeps q0's bits.  "base": True solves for the base pose too.  "damping" is lambda, in
[4e-3, 1e3]; "max_step" the largest joint update of one iteration in rad (float("inf"): none); "limits": True clamps the moving joints to the
model's limits after every update.  "target_frame": "world", or "root" for target positions given as offsets from the base position.

    targets                   [N, K, 7]: position, quaternion xyzw; allocated once (positions 0, identity quaternions): copy_ into it
    targets_from_bodies()     fills `targets` with the bodies' poses in the current state (one dwb launch): a problem solved by no update
    solve(targets=None, q0=None)
                              copies targets [N, K, 7] into `targets` and q0 [N, 33] into `q0` when given, one launch; returns `q`.  q0
                              None: the iteration starts from dof_state's positions
    refresh()                 one launch for `targets` as they stand, from dof_state's positions
    q, root                   [N, 33], [N, 7]: the solved angles, the base pose (root_states' bits with "base": False)
    residual, err             [N, m], [N, 2]: the error rows at `q` (position rows in m, orientation rows as rotation vectors in rad), their
                              largest active position and orientation words
    iters, converged          [N] int32, [N] uint8: updates applied, and whether `q` meets tol_pos and tol_ang
    dof_mask, dofs            [33] bool and the Gym DoF ids that may move
    names, index(name)        the targets' body names, and a name's target

A target quaternion whose norm is outside [0.99, 1.01], or a NaN, makes that env's outputs NaN and its `converged` 0, that env only.
"auto": True calls refresh() after every step(), after reset_idx() and reset().
"""
from __future__ import annotations

import math

import numpy as np

from . import cbind
from . import contact_dynamics as CM
from . import contact_inverse_dynamics as IM
from . import jacobians as JM
from .model_tensors import ModelTensor, resolve_front

HEADER = "dyros_inverse_kinematics.h"
NAME = "inverse_kinematics"
K = cbind.constants(HEADER, "dwq_")
EXPORTS = list(cbind.signatures(HEADER, "dwq_"))
DwqParams = cbind.structs(HEADER, "dwq_")["DwqParams"]
NB, NV, ND, GROUP, MAX_TARGETS, MAX_ITERATIONS, TABLE_WORDS = (K["DWQ_NUM_BODIES"], K["DWQ_NV"], K["DWQ_NUM_DOF"], K["DWQ_GROUP"], K["DWQ_MAX_TARGETS"],
                                                                K["DWQ_MAX_ITERATIONS"], K["DWQ_TABLE_WORDS"])
MIN_DAMPING, MAX_DAMPING = 4e-3, 1e3
ROWS = {"pose": (1, 1, 1, 1, 1, 1), "position": (1, 1, 1, 0, 0, 0), "orientation": (0, 0, 0, 1, 1, 1)}
FRAMES = ("world", "root")
DEFAULTS = {"targets": [{"body": "L_Foot_Link", "pos": [0.0, 0.0, -0.09]}, {"body": "R_Foot_Link", "pos": [0.0, 0.0, -0.09]}], "rows": None,
            "weights": None, "dofs": None, "base": False, "iterations": 16, "damping": 0.05, "max_step": 0.5, "tol_pos": 1e-5, "tol_ang": 1e-5,
            "limits": True, "target_frame": "world", "auto": False}


def declare(lib) -> dict:
    return cbind.declare(lib, HEADER, "dwq_")


def path_dofs(ids, body_moving, mv_parent) -> list:
    """The Gym DoFs on the paths from the base to the bodies `ids`, ascending (DoF j turns moving body j + 1)."""
    out = set()
    for g in ids:
        b = int(body_moving[g])
        while b > 0:
            out.add(b - 1)
            b = int(mv_parent[b])
    return sorted(out)


def params_struct(spec: dict) -> DwqParams:
    p = DwqParams()
    p.iterations, p.damping, p.max_step, p.tol_pos, p.tol_ang = spec["iterations"], spec["damping"], spec["max_step"], spec["tol_pos"], spec["tol_ang"]
    p.free_base, p.clamp_limits, p.targets_rel_root = int(spec["base"]), int(spec["limits"]), int(spec["target_frame"] == "root")
    return p


def pack_table(api: dict, model, ids, pos, row_mask=None, weights=None, dof_mask=None, lower=None, upper=None, params=None) -> np.ndarray:
    """The device table's DWQ_TABLE_WORDS words as a uint32 array (dwq_pack_table: dwj_pack_table's table, the targets, the row mask [6 K] or
    None for every row, the weights [6 K] or None for ones, the DoF mask [33] or None for every joint, the limits [33] (None: the model's) and
    params, a DwqParams or a dict of DEFAULTS' keys (None: the defaults); raises for what it refuses)."""
    import ctypes as C
    m = model if isinstance(model, JM.DwjModel) else JM.model_struct(model)
    c = ids if isinstance(ids, CM.DwcContacts) else CM.contacts_struct(ids, pos)
    n = 6 * max(1, min(c.count, MAX_TARGETS))

    def arr(x, dt, size, what):
        if x is None:
            return None
        a = np.ascontiguousarray(np.asarray(x, dt).reshape(-1))
        if a.size != size:
            raise ValueError("%s: %d %s where %d are read" % (NAME, a.size, what, size))
        return a
    rm, w, dm = arr(row_mask, np.uint8, n, "row mask words"), arr(weights, np.float32, n, "weights"), arr(dof_mask, np.uint8, ND, "DoF mask words")
    d = getattr(model, "d", model)
    lo = arr(d["dof_lower"] if lower is None else lower, np.float32, ND, "lower limits")
    hi = arr(d["dof_upper"] if upper is None else upper, np.float32, ND, "upper limits")
    p = params if isinstance(params, DwqParams) else params_struct(dict(DEFAULTS, **(params or {})))
    t = np.zeros(TABLE_WORDS, np.uint32)
    cbind.check(api, api["pack_table"](C.byref(m), C.byref(c), *(None if a is None else a.ctypes.data for a in (rm, w, dm)), lo.ctypes.data, hi.ctypes.data,
                                       C.byref(p), t.ctypes.data))
    return t


def _real(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and not math.isnan(v)


def resolve(spec, model=None) -> dict:
    """The cfg value as a full dict, plus "ids" and "pos" of the targets, "row_mask" [6 K], "w" (None or [6 K]), "dof_ids" and "dof_mask"
    [33]; None when the feature is off (None or False).  ValueError for anything else that is not True or a dict of the keys of DEFAULTS.
    model: the compiled model (None: the packaged one)."""
    out = resolve_front(NAME, spec, DEFAULTS, ("base", "limits", "auto"))
    if out is None:
        return None
    if model is None:
        from .model import load_model
        model = load_model()
    try:
        out["ids"], out["pos"] = CM.resolve_contacts(out["targets"], model.body_names, model.body_moving, NAME)
    except ValueError as e:
        raise ValueError(str(e).replace(".contacts", ".targets").replace("contact", "target")) from None
    k = len(out["ids"])
    rows = out["rows"]
    if rows is None:
        rows = ["pose"] * k
    if isinstance(rows, (str, bytes)) or not hasattr(rows, "__len__") or len(rows) != k or not all(isinstance(r, str) and r in ROWS for r in rows):
        raise ValueError("%s.rows must be None or %d of \"pose\", \"position\", \"orientation\", not %r" % (NAME, k, out["rows"]))
    out["row_mask"] = [b for r in rows for b in ROWS[r]]
    out["w"] = IM.resolve_weights(out["weights"], k, NAME)
    dof_names = list(model.dof_names)
    if out["dofs"] is None:
        ids = path_dofs(out["ids"], model.body_moving, model.mv_parent)
    else:
        d = out["dofs"]
        if isinstance(d, (str, bytes)) or not hasattr(d, "__len__") or not 1 <= len(d) <= ND:
            raise ValueError("%s.dofs must be None or a list of 1..%d DoF names or Gym DoF ids" % (NAME, ND))
        ids = []
        for j in d:
            if isinstance(j, str) and j in dof_names:
                ids.append(dof_names.index(j))
            elif isinstance(j, (int, np.integer)) and not isinstance(j, bool) and 0 <= int(j) < ND:
                ids.append(int(j))
            else:
                raise ValueError("%s.dofs: %r is neither a DoF name nor a Gym DoF id in 0..%d" % (NAME, j, ND - 1))
        if len(set(ids)) != len(ids):
            raise ValueError("%s.dofs names a joint twice" % NAME)
        ids = sorted(ids)
    out["dof_ids"], out["dof_mask"] = ids, [int(j in ids) for j in range(ND)]
    it = out["iterations"]
    if isinstance(it, bool) or not isinstance(it, (int, np.integer)) or not 1 <= it <= MAX_ITERATIONS:
        raise ValueError("%s.iterations must be an integer in 1..%d" % (NAME, MAX_ITERATIONS))
    if not _real(out["damping"]) or not MIN_DAMPING <= out["damping"] <= MAX_DAMPING:
        raise ValueError("%s.damping must be a number in [%g, %g]" % (NAME, MIN_DAMPING, MAX_DAMPING))
    if not _real(out["max_step"]) or not out["max_step"] > 0:
        raise ValueError("%s.max_step must be a positive number (float(\"inf\"): no limit)" % NAME)
    for k_ in ("tol_pos", "tol_ang"):
        if not _real(out[k_]) or not 0 <= out[k_] < math.inf:
            raise ValueError("%s.%s must be a finite number >= 0" % (NAME, k_))
    if out["target_frame"] not in FRAMES:
        raise ValueError("%s.target_frame must be \"world\" or \"root\"" % NAME)
    return out


def validate(spec) -> None:
    """Checks of cfg sim.mi355.inverse_kinematics (config.validate_cfg)."""
    resolve(spec)


class InverseKinematics(ModelTensor):
    """The joint angles that put bodies at poses, from one env object's bound buffers (see the module docstring).  host: a DyrosDynamicWalk
    (TocabiAMPLower hands its physics host).  Buffers are allocated here, once."""

    WHAT = "feature"

    def __init__(self, host, spec=True):
        import torch
        from . import body_states as BM
        model = host.model
        spec = resolve(spec, model)
        super().__init__(host, spec, declare)
        N = self.num_envs
        self.ids, self.pos = list(spec["ids"]), [list(p) for p in spec["pos"]]
        self.names = [model.body_names[g] for g in self.ids]
        self.num_targets = k = len(self.ids)
        m = self.rows = 6 * k
        self.dofs = list(spec["dof_ids"])
        self.dof_names = list(model.dof_names)
        self.rel_root = spec["target_frame"] == "root"
        self.table = self._upload(pack_table(self.api, model, self.ids, self.pos, spec["row_mask"], spec["w"], spec["dof_mask"], params=params_struct(spec)))
        self.dof_mask = torch.tensor(spec["dof_mask"], dtype=torch.bool, device=self._tdev)
        self.targets = self._zeros(N, k, 7)
        self.targets[..., 6] = 1.0
        self.q0 = self._zeros(N, ND)
        self.q, self.root = self._zeros(N, ND), self._zeros(N, 7)
        self.residual, self.err = self._zeros(N, m), self._zeros(N, 2)
        self.iters = torch.zeros(N, dtype=torch.int32, device=self._tdev)
        self.converged = torch.zeros(N, dtype=torch.uint8, device=self._tdev)
        outs = tuple(x.data_ptr() for x in (self.q, self.root, self.residual, self.err, self.iters, self.converged))
        self._args = self._inputs() + (None, self.targets.data_ptr()) + outs
        self._args_q0 = self._inputs() + (self.q0.data_ptr(), self.targets.data_ptr()) + outs
        # targets_from_bodies(): the bodies' rows by dwb_refresh at their origins, then the points
        import ctypes as C
        from . import _lib
        self._bapi = BM.declare(_lib.load()[0])
        self._btable = self._upload(BM.pack_table(self._bapi, model))
        self._bstates = self._zeros(N, k, BM.ROW)
        self._bids = (C.c_int32 * k)(*self.ids)
        self._broot = self._zeros(N, 13)          # (root_states at the origin: the bodies' rows then hold their offsets from the base)
        self._bargs = (N, self._btable.data_ptr(), self._broot.data_ptr(), self._in("dof_state", numel=N * 66), None, self._bids, k, 0,
                       self._bstates.data_ptr(), None)
        self._pos_t = torch.tensor(self.pos, dtype=torch.float32, device=self._tdev)

    def index(self, name: str) -> int:
        """The target (0 .. K - 1) on the body named."""
        if name not in self.names:
            raise ValueError("%s: no target on %r (targets: %s)" % (NAME, name, ", ".join(self.names)))
        return self.names.index(name)

    def targets_from_bodies(self):
        """Fills `targets` with the targets' poses in the current state: one dwb launch for the bodies' rows about a base at the origin, then each
        point's offset R pos, then (world frame) the base position.
        Solving for them is a problem with no update to make.  Returns `targets`."""
        import torch
        root = self.host._buf["root_states"].view(self.num_envs, 13)
        self._broot.copy_(root)
        self._broot[:, 0:3] = 0.0
        cbind.check(self._bapi, self._bapi["refresh"](*self._bargs, self._stream()))
        x, y, z, w = self._bstates[..., 3:7].unbind(-1)
        p = self._pos_t
        # R(q) pos, row by row
        rx = (1 - 2 * (y * y + z * z)) * p[:, 0] + 2 * (x * y - w * z) * p[:, 1] + 2 * (x * z + w * y) * p[:, 2]
        ry = 2 * (x * y + w * z) * p[:, 0] + (1 - 2 * (x * x + z * z)) * p[:, 1] + 2 * (y * z - w * x) * p[:, 2]
        rz = 2 * (x * z - w * y) * p[:, 0] + 2 * (y * z + w * x) * p[:, 1] + (1 - 2 * (x * x + y * y)) * p[:, 2]
        off = self._bstates[..., 0:3] + torch.stack([rx, ry, rz], -1)
        self.targets[..., 0:3] = off if self.rel_root else root[:, None, 0:3] + off
        self.targets[..., 3:7] = self._bstates[..., 3:7]
        return self.targets

    def refresh(self):
        """One launch on torch's current stream for `targets` as they stand, from dof_state's positions; returns `q`."""
        self._launch("solve", self._args)
        return self.q

    def solve(self, targets=None, q0=None):
        """Copies targets [N, K, 7] into `targets` and q0 [N, 33] into `q0` when given, one launch on torch's current stream; returns `q`
        [N, 33] and leaves `root`, `residual`, `err`, `iters` and `converged`.  q0 None: the iteration starts from dof_state's positions."""
        if targets is not None:
            self.targets.copy_(targets.reshape(self.targets.shape))
        if q0 is not None:
            self.q0.copy_(q0)
        self._launch("solve", self._args if q0 is None else self._args_q0)
        return self.q
