"""The contact-consistent dynamics (include/dyros_contact_dynamics.h, csrc/dw_contact_dynamics.hip): the equation of
motion under rigid contact constraints,  M nu_dot + h = b + J_c' f,  J_c nu_dot + Jd_c nu = gamma,  solved for nu_dot and f on the GPU in the
coordinates of isaacgymdyros_amd/jacobians.py.  One launch forms the contact Jacobian J_c and Jd_c nu, M and its L' D L factor
(forward_dynamics.py's, the same bits), Y = M^-1 J_c', A = J_c Y and its dense L D L', and solves.

Opt-in: cfg["sim"]["mi355"]["contact_dynamics"] = True, or {"contacts": [{"body": "L_Foot_Link", "pos": [0, 0, -0.09]}, {"body":
"R_Foot_Link", "pos": [0, 0, -0.09]}], "rhs": 1, "jacobian": True, "lambda": True, "lambda_inv": False, "minv_jt": False, "armature": True,
"auto": False}, gives a DyrosDynamicWalk env a `contact_dynamics` attribute (None otherwise; TocabiAMPLower: key `amp_contact_dynamics`).
Each call only reads the env's buffers, takes no argument that changes from call to call, allocates nothing and does not synchronise, so it
sits inside a captured rollout step.

A contact is a Gym body (name or id) and a point `pos` in that body's frame; 1 .. 4 contacts, no two on one moving body (a jointless body
stands for the moving body it is welded to).  Each contributes six rows in world axes: the point's linear velocity, then the body's angular
velocity; m = 6 K.  f is the wrench the environment applies to the robot at each contact point (force, then moment about the point, world
axes): the sign convention of force_sensors.  gamma is the contact frames' commanded acceleration; zero keeps the feet planted.

    forward_dynamics(tau_joint=None, gen_force=None, contact_accel=None)
                              returns `accel` [N, 39], the nu_dot that [0; tau_joint] + gen_force causes while the contacts accelerate
                              by contact_accel [N, m] (None: zero), and leaves the ground reaction in `force` [N, K, 6].  h comes from a
                              Dynamics launch of its own: two launches in all
    solve(rhs=None)           copies rhs [N, R, 39] (or [N, 39] when R = 1) into `rhs` when given, one launch with b = rhs and `gamma`;
                              returns `accel_all` [N, R, 39] and leaves `force_all` [N, R, m]
    refresh()                 one launch; fills `jc` and `jdnu`, `lambda_`, `lambda_inv`, `minv_jt` (those the spec holds)
    jc, jdnu                  [N, m, 39] and [N, m]: J_c and Jd_c nu ("jacobian")
    lambda_                   [N, m, m]: the contact-space inertia (J_c M^-1 J_c')^-1, symmetric bit for bit ("lambda")
    lambda_inv                [N, m, m]: J_c M^-1 J_c' ("lambda_inv")
    minv_jt                   [N, m, 39]: row r is M^-1 jc[r] ("minv_jt")
    rhs, gamma, accel_all, force_all
                              allocated once: copy_ into rhs and gamma so that no pointer ever changes
    names, index(name)        the contacts' body names, and a name's contact

From these, one bmm each: the dynamically consistent inverse  Jbar' = lambda_ @ minv_jt  [N, m, 39], and the contact null-space projector
N_c = I - minv_jt' lambda_ jc = torch.eye(39) - minv_jt.transpose(1, 2) @ lambda_ @ jc.  "rhs": R right-hand sides per env, 1 .. 8.
"armature": True forms M with the env's dof_armature.  "auto": True calls refresh() after every step(), after reset_idx() and reset().
"""
from __future__ import annotations

import math

import numpy as np

from . import cbind
from . import jacobians as JM
from .model_tensors import ModelTensor, joint_space_force, ptr, resolve_front

K = cbind.constants("dyros_contact_dynamics.h", "dwc_")
EXPORTS = list(cbind.signatures("dyros_contact_dynamics.h", "dwc_"))
DwcContacts = cbind.structs("dyros_contact_dynamics.h", "dwc_")["DwcContacts"]
NB, NV, GROUP, MAX_RHS, MAX_CONTACTS, TABLE_WORDS = (K["DWC_NUM_BODIES"], K["DWC_NV"], K["DWC_GROUP"], K["DWC_MAX_RHS"], K["DWC_MAX_CONTACTS"],
                                                     K["DWC_TABLE_WORDS"])
DEFAULTS = {"contacts": [{"body": "L_Foot_Link", "pos": [0.0, 0.0, -0.09]}, {"body": "R_Foot_Link", "pos": [0.0, 0.0, -0.09]}], "rhs": 1,
            "jacobian": True, "lambda": True, "lambda_inv": False, "minv_jt": False, "armature": True, "auto": False}


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_contact_dynamics.h", "dwc_")


def contacts_struct(ids, pos) -> DwcContacts:
    """DwcContacts from Gym ids and points [K][3]; what does not fit the struct is left for dwc_pack_table to refuse (a count outside 1..4)."""
    c = DwcContacts()
    c.count = len(ids)
    for i, (g, p) in enumerate(list(zip(ids, pos))[:MAX_CONTACTS]):
        c.body[i] = int(g)
        for k in range(3):
            c.pos[i][k] = float(p[k])
    return c


def pack_table(api: dict, model, ids, pos) -> np.ndarray:
    """The device table's DWC_TABLE_WORDS words as a uint32 array (dwc_pack_table: dwl_pack_table's table, then the contacts; raises for a
    model or contacts it refuses)."""
    import ctypes as C
    m, t = model if isinstance(model, JM.DwjModel) else JM.model_struct(model), np.zeros(TABLE_WORDS, np.uint32)
    c = ids if isinstance(ids, DwcContacts) else contacts_struct(ids, pos)
    cbind.check(api, api["pack_table"](C.byref(m), C.byref(c), t.ctypes.data))
    return t


def resolve_contacts(cs, names=None, carriers=None, name="contact_dynamics"):
    """(ids, pos) of a cfg's "contacts"; ValueError under the feature's `name` for what is no list of 1 .. 4 contacts on different moving bodies.
    names, carriers: the model's body names and body_moving (None: the packaged model's)."""
    if names is None or carriers is None:
        from .model import load_model
        model = load_model()
        names, carriers = model.body_names, model.body_moving
    names = list(names)
    if not isinstance(cs, (list, tuple)) or not 1 <= len(cs) <= MAX_CONTACTS:
        raise ValueError("%s.contacts must be a list of 1..%d contacts" % (name, MAX_CONTACTS))
    ids, pos = [], []
    for c in cs:
        if not isinstance(c, dict) or "body" not in c or set(c) - {"body", "pos"}:
            raise ValueError("%s.contacts: a contact is {\"body\": name or Gym id, \"pos\": [x, y, z]}, not %r" % (name, c))
        b = c["body"]
        if isinstance(b, str):
            if b not in names:
                raise ValueError("%s.contacts: no body named %r" % (name, b))
            ids.append(names.index(b))
        elif isinstance(b, (int, np.integer)) and not isinstance(b, bool) and 0 <= int(b) < len(names):
            ids.append(int(b))
        else:
            raise ValueError("%s.contacts: %r is neither a body name nor a Gym id in 0..%d" % (name, b, len(names) - 1))
        p = c.get("pos", [0.0, 0.0, 0.0])
        if (isinstance(p, (str, bytes)) or not hasattr(p, "__len__") or len(p) != 3
                or not all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v) for v in p)):
            raise ValueError("%s.contacts: pos must be three finite numbers, not %r" % (name, p))
        pos.append([float(v) for v in p])
    moving = [int(carriers[g]) for g in ids]
    if len(set(moving)) != len(moving):
        raise ValueError("%s.contacts: two contacts on one moving body: their rows would be dependent" % name)
    return ids, pos


def resolve(spec, names=None, carriers=None) -> dict:
    """The cfg value as a full dict, plus "ids" and "pos" of the contacts; None when the feature is off (None or False).  ValueError for
    anything else that is not True or a dict of the keys of DEFAULTS.  names, carriers: the model's body names and body_moving (None: the
    packaged model's)."""
    out = resolve_front("contact_dynamics", spec, DEFAULTS, ("jacobian", "lambda", "lambda_inv", "minv_jt", "armature", "auto"))
    if out is None:
        return None
    if isinstance(out["rhs"], bool) or not isinstance(out["rhs"], int) or not 1 <= out["rhs"] <= MAX_RHS:
        raise ValueError("contact_dynamics.rhs must be an integer in 1..%d" % MAX_RHS)
    out["ids"], out["pos"] = resolve_contacts(out["contacts"], names, carriers)
    return out


def validate(spec) -> None:
    """Checks of cfg sim.mi355.contact_dynamics (config.validate_cfg)."""
    resolve(spec)


class ContactDynamics(ModelTensor):
    """The contact Jacobian, the contact-space inertia and the constrained forward dynamics of one env object's bound buffers (see the module
    docstring).  host: a DyrosDynamicWalk (TocabiAMPLower hands its physics host); vel_at_com: the host's root_vel_at_com unless given.
    Buffers are allocated here, once."""

    WHAT = "feature"

    def __init__(self, host, spec=True, vel_at_com=None):
        from .dynamics import Dynamics
        model = host.model
        spec = resolve(spec, model.body_names, model.body_moving)
        super().__init__(host, spec, declare)
        N, R = self.num_envs, spec["rhs"]
        self.nrhs = R
        self.ids, self.pos = list(spec["ids"]), [list(p) for p in spec["pos"]]
        self.names = [model.body_names[g] for g in self.ids]
        self.num_contacts = len(self.ids)
        m = self.rows = 6 * self.num_contacts
        self.dof_names = list(model.dof_names)
        self.vel_at_com = self._vel_at_com(vel_at_com)
        self.table = self._upload(pack_table(self.api, model, self.ids, self.pos))
        self.jc = self._zeros(N, m, NV) if spec["jacobian"] else None
        self.jdnu = self._zeros(N, m) if spec["jacobian"] else None
        self.lambda_ = self._zeros(N, m, m) if spec["lambda"] else None
        self.lambda_inv = self._zeros(N, m, m) if spec["lambda_inv"] else None
        self.minv_jt = self._zeros(N, m, NV) if spec["minv_jt"] else None
        self.rhs = self._zeros(N, R, NV)
        self.gamma = self._zeros(N, m)
        self.accel_all = self._zeros(N, R, NV)
        self.force_all = self._zeros(N, R, m)
        # forward_dynamics(): a right-hand side, a gamma and solutions of its own, and h from a Dynamics of its own (bias alone, one launch)
        self._fd_rhs = self._zeros(N, 1, NV)
        self._fd_gamma = self._zeros(N, m)
        self.accel = self._zeros(N, NV)
        self.force = self._zeros(N, self.num_contacts, 6)
        self._bias = Dynamics(host, {"bias": True, "gravity": False}, vel_at_com=self.vel_at_com)
        common = self._inputs(spec["armature"]) + (self.vel_at_com,)
        none5 = (None,) * 5
        self._solve_args = common + (self.rhs.data_ptr(), R, None, self.gamma.data_ptr()) + none5 + (self.accel_all.data_ptr(), self.force_all.data_ptr())
        self._fd_args = common + (self._fd_rhs.data_ptr(), 1, self._bias.bias.data_ptr(), self._fd_gamma.data_ptr()) + none5 + (self.accel.data_ptr(),
                                                                                                                                  self.force.data_ptr())
        outs = (ptr(self.jc), ptr(self.jdnu), ptr(self.minv_jt), ptr(self.lambda_inv), ptr(self.lambda_))
        self._refresh_args = common + (None, 0, None, None) + outs + (None, None) if any(o is not None for o in outs) else None

    def index(self, name: str) -> int:
        """The contact (0 .. K - 1) on the body named."""
        if name not in self.names:
            raise ValueError("contact_dynamics: no contact on %r (contacts: %s)" % (name, ", ".join(self.names)))
        return self.names.index(name)

    def refresh(self):
        """One launch on torch's current stream: `jc`, `jdnu`, `lambda_`, `lambda_inv` and `minv_jt`, those the spec holds (none: no launch)."""
        if self._refresh_args is not None:
            self._launch("solve", self._refresh_args)

    def solve(self, rhs=None):
        """The constrained solve of b = rhs with `gamma`: copies rhs [N, R, 39] (R = 1: [N, 39] too) into `rhs` when given, one launch on torch's
        current stream; returns `accel_all` [N, R, 39] and leaves `force_all` [N, R, m]."""
        if rhs is not None:
            self.rhs.copy_(rhs.reshape(self.rhs.shape))
        self._launch("solve", self._solve_args)
        return self.accel_all

    def forward_dynamics(self, tau_joint=None, gen_force=None, contact_accel=None):
        """accel = the nu_dot of b = [0; tau_joint] + gen_force - h under the contacts, which accelerate by contact_accel [N, m] (None: zero):
        tau_joint [N, 33] and gen_force [N, 39], each or None (zero).  Two launches on torch's current stream, the bias forces and the solve;
        returns `accel` [N, 39] and leaves the ground reaction in `force` [N, K, 6]."""
        joint_space_force(self._fd_rhs[:, 0], tau_joint, gen_force)
        if contact_accel is not None:
            self._fd_gamma.copy_(contact_accel.reshape(self._fd_gamma.shape))
        else:
            self._fd_gamma.zero_()
        self._bias.refresh()
        self._launch("solve", self._fd_args)
        return self.accel
