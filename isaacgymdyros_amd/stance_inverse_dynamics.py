"""The stance inverse dynamics (include/dyros_stance_inverse_dynamics.h, csrc/dw_contact_inverse.hip):
contact_inverse_dynamics.py's question -- the joint torques and contact wrenches that give the robot a wanted acceleration, M a + h = [0;
tau_joint] + J_c' f -- asked per env for the contacts that env stands on, with the distance of every loaded contact from what a sole can
deliver.  A rollout holds envs in double support, in single support on either foot and in flight at once; `stance` [N, K] says which of the
K contacts carry load in each env, and one launch solves every env over its own contact set.  All-ones is contact_inverse_dynamics, bit for
bit.

Opt-in: cfg["sim"]["mi355"]["stance_inverse_dynamics"] = True, or {"contacts": [contact_inverse_dynamics.py's default], "weights": None,
"soles": "model", "friction": 1.0, "contact_accel": True, "margins": True, "base_residual": True, "tau_full": False, "armature": True,
"auto": False}, gives a DyrosDynamicWalk env a `stance_inverse_dynamics` attribute (None otherwise; TocabiAMPLower: key
`amp_stance_inverse_dynamics`).  Each call only reads the env's buffers, takes no argument that changes from call to call, allocates nothing
and does not synchronise, so it sits inside a captured rollout step.  Plane only: the sole normal stands for the ground's, and a cfg with
height-field terrain is refused.

Contacts and "weights" are contact_inverse_dynamics.py's.  "soles": "model" gives a contact on a foot the bounding rectangle of the model's
four sole corners (centre [0.03, 0, -0.1585], half extents [0.15, 0.085], in the ankle link's frame) and any other contact a point; or a
list of K entries, each {"center": [3], "half": [2]} or None (a point at the contact's pos, which carries no moment).  "friction": mu.

    solve(accel=None, force_ref=None, stance=None)
                              copies what it is given into `accel`, `force_ref` and `stance`, one launch; returns `tau_joint`
    refresh()                 one launch for the buffers as they stand
    stance_from_phase()       DyrosDynamicWalk only: the stance of the contacts on the two feet from the env's mocap_data_idx with the
                              reward's windows (300 <= idx < 1500: right foot only; 2100 <= idx < 3300: left foot only; else both); other
                              contacts stay as they stand.  torch ops only: capturable
    stance_from_load(threshold)
                              a contact is active where its body's row of the env's contact_forces has F_z > threshold
    stance                    [N, K] uint8, allocated once (ones)
    accel, force_ref          [N, 39] and [N, m], allocated once (zeros)
    tau_joint                 [N, 33]
    force, force_all          [N, K, 6], a view of [N, m]; an inactive contact's wrench is +0.0
    contact_accel, tau_full   [N, m], [N, 39], as contact_inverse_dynamics's: the stance does not enter
    base_residual             [N, 6]: the base rows' r[0:6] - J_b' f: rounding on a stance that is not empty, the whole of r[0:6] in flight
    margins                   [N, K, 4]: normal force, friction cone, centre of pressure along the sole's x and its y; each >= 0 exactly when
                              the sole can deliver the wrench; +0.0 for an inactive contact
    feasible                  [N] uint8: 1 when the stance is not empty and every margin of every active contact is >= 0
    names, index(name)        the contacts' body names, and a name's contact
"""
from __future__ import annotations

import math

import numpy as np

from . import cbind
from . import contact_inverse_dynamics as IM
from .model_tensors import ptr, resolve_front

K = cbind.constants("dyros_stance_inverse_dynamics.h", "dwk_")
EXPORTS = list(cbind.signatures("dyros_stance_inverse_dynamics.h", "dwk_"))
NB, NV, ND, GROUP, MAX_CONTACTS, TABLE_WORDS = K["DWK_NUM_BODIES"], K["DWK_NV"], K["DWK_NUM_DOF"], K["DWK_GROUP"], K["DWK_MAX_CONTACTS"], K["DWK_TABLE_WORDS"]
SOLE_WORDS, MARGINS = K["DWK_SOLE_WORDS"], K["DWK_MARGINS"]
DEFAULTS = {"contacts": [dict(c, pos=list(c["pos"])) for c in IM.DEFAULTS["contacts"]], "weights": None, "soles": "model", "friction": 1.0,
            "contact_accel": True, "margins": True, "base_residual": True, "tau_full": False, "armature": True, "auto": False}
RSSP, LSSP = (300, 1500), (2100, 3300)          # csrc/dw_gait.h's window_of: right foot only, left foot only; else both
NAME = "stance_inverse_dynamics"


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_stance_inverse_dynamics.h", "dwk_")


def pack_table(api: dict, model, ids, pos, weights=None, soles=None, mu=1.0) -> np.ndarray:
    """The device table's DWK_TABLE_WORDS words as a uint32 array (dwk_pack_table: dwi_pack_table's table, then the soles [K, 5] -- None:
    points at the contacts' pos -- and mu; raises for what it refuses)."""
    import ctypes as C
    (m, c, w, n), t = IM.table_front(model, ids, pos, weights, NAME), np.zeros(TABLE_WORDS, np.uint32)
    s = None if soles is None else np.ascontiguousarray(np.asarray(soles, np.float32).reshape(-1))
    if s is not None and s.size != SOLE_WORDS * n:
        raise ValueError("%s: %d sole words for %d contacts" % (NAME, s.size, c.count))
    cbind.check(api, api["pack_table"](C.byref(m), C.byref(c), None if w is None else w.ctypes.data, None if s is None else s.ctypes.data, float(mu), t.ctypes.data))
    return t


def model_soles(model=None) -> dict:
    """moving body -> [cx, cy, cz, hx, hy]: the bounding rectangle of each foot's four sole corners (the model's foot_pts)."""
    if model is None:
        from .model import load_model
        model = load_model()
    d, out = getattr(model, "d", model), {}
    for mv in dict.fromkeys(f["moving"] for f in d["foot_pts"]):
        p = np.array([f["pos"] for f in d["foot_pts"] if f["moving"] == mv], np.float64)
        lo, hi = p.min(0), p.max(0)
        out[int(mv)] = [round(float(x), 9) + 0.0 for x in ((lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, hi[2], (hi[0] - lo[0]) / 2, (hi[1] - lo[1]) / 2)]
    return out


def _numbers(v, n, lo=None) -> bool:
    return (not isinstance(v, (str, bytes)) and hasattr(v, "__len__") and len(v) == n
            and all(isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool) and math.isfinite(x) and (lo is None or x >= lo) for x in v))


def resolve_soles(soles, ids, pos, model=None):
    """[K][5] floats: "model", or K entries of {"center": [3], "half": [2]} or None.  ValueError otherwise."""
    count = len(ids)
    bad = ValueError('%s.soles must be "model" or %d entries, each None or {"center": three finite numbers, "half": two finite numbers >= 0}, not %r'
                     % (NAME, count, soles))
    point = lambda i: [float(x) for x in pos[i]] + [0.0, 0.0]          # noqa: E731
    if isinstance(soles, str):
        if soles != "model":
            raise bad
        if model is None:
            from .model import load_model
            model = load_model()
        by_mv, moving = model_soles(model), getattr(model, "d", model)["body_moving"]
        return [list(by_mv[moving[g]]) if moving[g] in by_mv else point(i) for i, g in enumerate(ids)]
    if isinstance(soles, (bytes, dict)) or not hasattr(soles, "__len__") or len(soles) != count:
        raise bad
    out = []
    for i, s in enumerate(soles):
        if s is None:
            out.append(point(i))
        elif isinstance(s, dict) and set(s) == {"center", "half"} and _numbers(s["center"], 3) and _numbers(s["half"], 2, 0.0):
            out.append([float(x) for x in s["center"]] + [float(x) for x in s["half"]])
        else:
            raise bad
    return out


def resolve(spec, model=None, terrain=None) -> dict:
    """The cfg value as a full dict, plus "ids", "pos", "w" (contact_inverse_dynamics.resolve's) and "sole_words" [K][5]; None when the
    feature is off (None or False).  ValueError for anything else that is not True or a dict of the keys of DEFAULTS, and for terrain: a
    cfg["terrain"] whose mesh_type is a height field.  model: a TocabiModel (None: the packaged one)."""
    out = resolve_front(NAME, spec, DEFAULTS, ("contact_accel", "margins", "base_residual", "tau_full", "armature", "auto"))
    if out is None:
        return None
    if dict(terrain or {}).get("mesh_type", "plane") in ("heightfield", "trimesh"):
        raise ValueError("%s: plane only -- the sole normal stands for the ground's (include/dyros_stance_inverse_dynamics.h)" % NAME)
    names, carriers = (None, None) if model is None else (model.body_names, model.body_moving)
    IM.resolve_contacts(out, names, carriers, NAME)
    mu = out["friction"]
    if not (isinstance(mu, (int, float, np.integer, np.floating)) and not isinstance(mu, bool) and math.isfinite(mu) and mu > 0):
        raise ValueError("%s.friction must be a finite positive number, not %r" % (NAME, mu))
    out["friction"] = float(mu)
    out["sole_words"] = resolve_soles(out["soles"], out["ids"], out["pos"], model)
    return out


def validate(spec, terrain=None) -> None:
    """Checks of cfg sim.mi355.stance_inverse_dynamics (config.validate_cfg)."""
    resolve(spec, terrain=terrain)


def phase_stance(idx):
    """(left, right) of a mocap row index (int or array): the reward's windows of csrc/dw_gait.h."""
    rssp, lssp = (RSSP[0] <= idx) & (idx < RSSP[1]), (LSSP[0] <= idx) & (idx < LSSP[1])
    return ~rssp, ~lssp


class StanceInverseDynamics(IM.ContactInverseDynamics):
    """The joint torques and contact wrenches of a wanted acceleration under each env's stance, with the soles' margins, from one env
    object's bound buffers (see the module docstring).  host: a DyrosDynamicWalk (TocabiAMPLower hands its physics host); vel_at_com: the
    host's root_vel_at_com unless given.  Buffers are allocated here, once."""

    NAME = NAME
    task_host = True          # the host's task state is the env's (model_tensors.attach: False under TocabiAMPLower, whose host only carries the physics)
    _declare = staticmethod(declare)

    @staticmethod
    def _resolve(spec, model):
        return resolve(spec, model)

    def _pack(self, model):
        return pack_table(self.api, model, self.ids, self.pos, self.weights, self.soles, self.friction)

    def _extra(self, spec):
        import torch
        N, Kc = self.num_envs, self.num_contacts
        self.soles, self.friction = [list(s) for s in spec["sole_words"]], spec["friction"]
        self.stance = torch.ones(N, Kc, dtype=torch.uint8, device=self._tdev)
        self.base_residual = self._zeros(N, 6) if spec["base_residual"] else None
        self.margins = self._zeros(N, Kc, MARGINS) if spec["margins"] else None
        self.feasible = torch.zeros(N, dtype=torch.uint8, device=self._tdev)

    def _arguments(self, accel, force_ref, outputs) -> tuple:
        return (accel, force_ref, self.stance.data_ptr(), self.vel_at_com) + outputs + (ptr(self.base_residual), ptr(self.margins), self.feasible.data_ptr())

    def __init__(self, host, spec=True, vel_at_com=None):
        if getattr(host, "custom_origins", False):
            raise ValueError("%s: plane only (include/dyros_stance_inverse_dynamics.h); this env runs on a height field" % NAME)
        super().__init__(host, spec, vel_at_com)
        # the contacts on the two feet's moving bodies, for stance_from_phase
        d = getattr(host.model, "d", host.model)
        feet = list(dict.fromkeys(f["moving"] for f in d["foot_pts"]))
        self._foot_contact = [next((i for i, g in enumerate(self.ids) if d["body_moving"][g] == mv), None) for mv in feet]          # (left, right)
        self._idx = self._forces = None

    def solve(self, accel=None, force_ref=None, stance=None):
        """Copies accel [N, 39], force_ref [N, m] or [N, K, 6] and stance [N, K] into the buffers when given, one launch on torch's current
        stream; returns `tau_joint` [N, 33] and leaves the other outputs."""
        if stance is not None:
            self.stance.copy_(stance.reshape(self.stance.shape) != 0)
        return super().solve(accel, force_ref)

    def stance_from_phase(self):
        """`stance` of the contacts on the left and the right foot from the env's mocap_data_idx (see the module docstring); returns
        `stance`.  DyrosDynamicWalk only: no other task has the gait's phase."""
        if not self.task_host or "env_state" not in getattr(self.host, "_buf", {}):
            raise ValueError("%s.stance_from_phase: DyrosDynamicWalk only -- this env's task has no mocap_data_idx" % NAME)
        if self._idx is None:
            from . import abi
            self._idx = abi.es_view(self.host._buf["env_state"], "mocap_data_idx")[:, 0]
        for on, c in zip(phase_stance(self._idx), self._foot_contact):
            if c is not None:
                self.stance[:, c].copy_(on)
        return self.stance

    def stance_from_load(self, threshold: float = 0.0):
        """`stance`: a contact is active where its body's row of the env's contact_forces [N, 38, 3] has F_z > threshold; returns `stance`."""
        if self._forces is None:
            self._forces = self.host._buf["contact_forces"].view(self.num_envs, NB, 3)
        for c, g in enumerate(self.ids):
            self.stance[:, c].copy_(self._forces[:, g, 2] > threshold)
        return self.stance
