"""The contact inverse dynamics (include/dyros_contact_inverse_dynamics.h, csrc/dw_contact_inverse.hip): the joint torques
and the contact wrenches that give the robot a wanted acceleration while its contacts carry the floating base,
M a + h = [0; tau_joint] + J_c' f,  solved for tau_joint and f on the GPU in the coordinates of isaacgymdyros_amd/jacobians.py.  It is the
inverse question to contact_dynamics.py's: that one takes a torque and returns the acceleration and the ground reaction.  One launch forms
r = M a + h (dynamics.py's recursion, the same bits), the base columns J_b of the contact Jacobian, G = J_b' W^-1 J_b and its L D L', the
wrenches f = f_ref + W^-1 J_b G^-1 (r[0:6] - J_b' f_ref) and tau_joint = r[6:] - J_j' f.  Nothing needs M or its factor.

Opt-in: cfg["sim"]["mi355"]["contact_inverse_dynamics"] = True, or {"contacts": [{"body": "L_Foot_Link", "pos": [0, 0, -0.09]}, {"body":
"R_Foot_Link", "pos": [0, 0, -0.09]}], "weights": None, "contact_accel": True, "tau_full": False, "armature": True, "auto": False}, gives a
DyrosDynamicWalk env a `contact_inverse_dynamics` attribute (None otherwise; TocabiAMPLower: key `amp_contact_inverse_dynamics`).  Each call
only reads the env's buffers, takes no argument that changes from call to call, allocates nothing and does not synchronise, so it sits
inside a captured rollout step.

Contacts are contact_dynamics.py's: a Gym body (name or id) and a point `pos` in its frame; 1 .. 4 contacts, no two on one moving body;
six rows each, m = 6 K.  f is the wrench the environment applies to the robot at each contact point (force, then moment about the point, world
axes).  f is the wrench set closest to `force_ref` in the norm of "weights" that carries the base rows exactly: J_b' f = r[0:6].  "weights":
None (ones), six positive numbers (every contact's: forces, then moments) or K lists of six; larger weights make a row dearer.  With one
contact f is unique and the weights do not enter.

Whether the contacts can deliver f -- unilateral, inside the friction cone, the centre of pressure inside the sole -- is NOT decided here:
read it from `force`.

    solve(accel=None, force_ref=None)
                              copies accel [N, 39] into `accel` and force_ref [N, m] (or [N, K, 6]) into `force_ref` when given, one
                              launch; returns `tau_joint` [N, 33] and leaves `force`, `contact_accel` and `tau_full`
    refresh()                 one launch for the buffers as they stand
    accel, force_ref          [N, 39] and [N, m], allocated once (zeros): copy_ into them so that no pointer ever changes.  accel = 0 asks
                              for the torques and wrenches that hold nu_dot = 0
    tau_joint                 [N, 33]
    force, force_all          [N, K, 6], a view of [N, m]
    contact_accel             [N, m]: J_c accel + Jd_c nu, the contact frames' acceleration under accel ("contact_accel")
    tau_full                  [N, 39]: M accel + h ("tau_full")
    names, index(name)        the contacts' body names, and a name's contact

Round trip: contact_dynamics.forward_dynamics(tau_joint, contact_accel=contact_accel) returns `accel` and `force` again.  "armature": True
forms r with the env's dof_armature.  "auto": True calls refresh() after every step(), after reset_idx() and reset().  The gravity vector is
the cfg's sim.gravity.
"""
from __future__ import annotations

import math

import numpy as np

from . import cbind
from . import contact_dynamics as CM
from . import jacobians as JM
from .model_tensors import ModelTensor, ptr, resolve_front

K = cbind.constants("dyros_contact_inverse_dynamics.h", "dwi_")
EXPORTS = list(cbind.signatures("dyros_contact_inverse_dynamics.h", "dwi_"))
NB, NV, ND, GROUP, MAX_CONTACTS, TABLE_WORDS = K["DWI_NUM_BODIES"], K["DWI_NV"], K["DWI_NUM_DOF"], K["DWI_GROUP"], K["DWI_MAX_CONTACTS"], K["DWI_TABLE_WORDS"]
DEFAULTS = {"contacts": [{"body": "L_Foot_Link", "pos": [0.0, 0.0, -0.09]}, {"body": "R_Foot_Link", "pos": [0.0, 0.0, -0.09]}], "weights": None,
            "contact_accel": True, "tau_full": False, "armature": True, "auto": False}
NAME = "contact_inverse_dynamics"          # in the messages; stance_inverse_dynamics.py passes its own


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_contact_inverse_dynamics.h", "dwi_")


def table_front(model, ids, pos, weights, name=NAME):
    """What a pack_table of this table begins with: the model and the contacts as structs, the weights as [6 K] float32 or None (ValueError
    for another size) and the count they were sized for."""
    m = model if isinstance(model, JM.DwjModel) else JM.model_struct(model)
    c = ids if isinstance(ids, CM.DwcContacts) else CM.contacts_struct(ids, pos)
    n = max(1, min(c.count, MAX_CONTACTS))
    w = None if weights is None else np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
    if w is not None and w.size != 6 * n:
        raise ValueError("%s: %d weights for %d contacts" % (name, w.size, c.count))
    return m, c, w, n


def pack_table(api: dict, model, ids, pos, weights=None) -> np.ndarray:
    """The device table's DWI_TABLE_WORDS words as a uint32 array (dwi_pack_table: dwn_pack_table's table, the contacts, the weights [6 K] or
    None for ones; raises for a model, contacts or weights it refuses)."""
    import ctypes as C
    (m, c, w, _), t = table_front(model, ids, pos, weights), np.zeros(TABLE_WORDS, np.uint32)
    cbind.check(api, api["pack_table"](C.byref(m), C.byref(c), None if w is None else w.ctypes.data, t.ctypes.data))
    return t


def _number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v) and v > 0


def resolve_weights(weights, count: int, name=NAME):
    """None, or the weights as [6 K] floats: six positive numbers (every contact's) or K lists of six.  ValueError otherwise."""
    if weights is None:
        return None
    bad = ValueError("%s.weights must be None, six finite positive numbers or %d lists of six, not %r" % (name, count, weights))
    if isinstance(weights, (str, bytes)) or not hasattr(weights, "__len__") or len(weights) == 0:
        raise bad
    rows = list(weights)
    if all(_number(v) for v in rows):
        if len(rows) != 6:
            raise bad
        return [float(v) for v in rows] * count
    if len(rows) != count or not all(not isinstance(r, (str, bytes)) and hasattr(r, "__len__") and len(r) == 6 and all(_number(v) for v in r) for r in rows):
        raise bad
    return [float(v) for r in rows for v in r]


def resolve_contacts(out: dict, names=None, carriers=None, name=NAME) -> dict:
    """out with "ids" and "pos" of its "contacts" and "w" (None or [6 K]) of its "weights"; ValueError under `name`."""
    out["ids"], out["pos"] = CM.resolve_contacts(out["contacts"], names, carriers, name)
    out["w"] = resolve_weights(out["weights"], len(out["ids"]), name)
    return out


def resolve(spec, names=None, carriers=None) -> dict:
    """The cfg value as a full dict, plus "ids" and "pos" of the contacts and "w" (None or [6 K]); None when the feature is off (None or
    False).  ValueError for anything else that is not True or a dict of the keys of DEFAULTS.  names, carriers: the model's body names and
    body_moving (None: the packaged model's)."""
    out = resolve_front(NAME, spec, DEFAULTS, ("contact_accel", "tau_full", "armature", "auto"))
    return None if out is None else resolve_contacts(out, names, carriers)


def validate(spec) -> None:
    """Checks of cfg sim.mi355.contact_inverse_dynamics (config.validate_cfg)."""
    resolve(spec)


class ContactInverseDynamics(ModelTensor):
    """The joint torques and contact wrenches of a wanted acceleration, from one env object's bound buffers (see the module docstring).  host:
    a DyrosDynamicWalk (TocabiAMPLower hands its physics host); vel_at_com: the host's root_vel_at_com unless given.  Buffers are allocated
    here, once.  A subclass over another ABI of the same launch (stance_inverse_dynamics.py) gives NAME and the hooks below."""

    WHAT = "feature"
    NAME = NAME

    # ---- what differs between the ABIs ----
    _declare = staticmethod(declare)

    @staticmethod
    def _resolve(spec, model):
        return resolve(spec, model.body_names, model.body_moving)

    def _pack(self, model):
        """The packed table."""
        return pack_table(self.api, model, self.ids, self.pos, self.weights)

    def _extra(self, spec):
        """The buffers beyond the common ones."""

    def _arguments(self, accel, force_ref, outputs) -> tuple:
        """The entry point's arguments after the gravity vector, in the ABI's order."""
        return (accel, force_ref, self.vel_at_com) + outputs

    def __init__(self, host, spec=True, vel_at_com=None):
        model = host.model
        spec = self._resolve(spec, model)
        super().__init__(host, spec, self._declare)
        N = self.num_envs
        self.ids, self.pos = list(spec["ids"]), [list(p) for p in spec["pos"]]
        self.names = [model.body_names[g] for g in self.ids]
        self.num_contacts = len(self.ids)
        m = self.rows = 6 * self.num_contacts
        self.weights = None if spec["w"] is None else list(spec["w"])
        self.dof_names = list(model.dof_names)
        self.vel_at_com = self._vel_at_com(vel_at_com)
        self.g = tuple(float(x) for x in host.cfg["sim"].get("gravity", [0.0, 0.0, -9.81]))
        if len(self.g) != 3 or not all(math.isfinite(x) for x in self.g):
            raise ValueError("%s: sim.gravity must be three finite numbers" % self.NAME)
        self._extra(spec)
        self.table = self._upload(self._pack(model))
        self.accel = self._zeros(N, NV)
        self.force_ref = self._zeros(N, m)
        self.tau_joint = self._zeros(N, ND)
        self.force_all = self._zeros(N, m)
        self.force = self.force_all.view(N, self.num_contacts, 6)
        self.contact_accel = self._zeros(N, m) if spec["contact_accel"] else None
        self.tau_full = self._zeros(N, NV) if spec["tau_full"] else None
        self._args = self._inputs(spec["armature"]) + self.g + self._arguments(
            self.accel.data_ptr(), self.force_ref.data_ptr(), (self.tau_joint.data_ptr(), self.force_all.data_ptr(), ptr(self.contact_accel), ptr(self.tau_full)))

    def index(self, name: str) -> int:
        """The contact (0 .. K - 1) on the body named."""
        if name not in self.names:
            raise ValueError("%s: no contact on %r (contacts: %s)" % (self.NAME, name, ", ".join(self.names)))
        return self.names.index(name)

    def refresh(self):
        """One launch on torch's current stream for the input buffers as they stand (`accel` and `force_ref`; under a stance also `stance`):
        `tau_joint`, `force`, and the other outputs where the spec holds them."""
        self._launch("solve", self._args)

    def solve(self, accel=None, force_ref=None):
        """Copies accel [N, 39] into `accel` and force_ref [N, m] or [N, K, 6] into `force_ref` when given, one launch on torch's current
        stream; returns `tau_joint` [N, 33] and leaves `force` [N, K, 6]."""
        if accel is not None:
            self.accel.copy_(accel)
        if force_ref is not None:
            self.force_ref.copy_(force_ref.reshape(self.force_ref.shape))
        self._launch("solve", self._args)
        return self.tau_joint
