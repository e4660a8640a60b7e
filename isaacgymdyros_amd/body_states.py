"""The rigid-body state tensor (include/dyros_bodies.h, csrc/dw_bodies.hip): Isaac Gym's
acquire_rigid_body_state_tensor / refresh_rigid_body_state_tensor for the 38 TOCABI bodies.

Opt-in: cfg["sim"]["mi355"]["body_states"] = True, or {"bodies": [names or Gym ids], "com": True, "auto": False}, gives a
DyrosDynamicWalk env a `body_states` attribute (None otherwise; TocabiAMPLower: key `amp_body_states`).  refresh() makes one launch,
dwb_refresh, on torch's current stream: position, quaternion xyzw, linear and angular velocity of every chosen body in the world frame, from
the bound root_states and dof_state by the physics' own chain, and the centre of mass.  It only reads the env's buffers, takes no argument
that changes from call to call, allocates nothing and does not synchronise, so it sits inside a captured rollout step.

    refresh()                 one launch; returns `states` [N, K, 13]
    pos, rot, vel, ang_vel    views of `states`: [N, K, 3], [N, K, 4], [N, K, 3], [N, K, 3]
    com                       [N, 7]: centre of mass, its velocity, the total mass (None with "com": False)
    names, parents, ids       of the K rows; parents: the row of the Gym parent body within the selection, or -1
    index(name), rows(*names)

"auto": True refreshes after every step() (after the step's launch, before the run trace and the gait profile record), after reset_idx()
and reset().  Row 0 (base_link) is the root row bit for bit.  The linear velocity of a body is its COM's when the env's root_vel_at_com is
set (the default, as PhysX reports it) and its origin's otherwise; Gym bodies 7 and 15 have no inertial record and always give the origin's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import cbind
from .model_tensors import ModelTensor, ptr, resolve_front

K = cbind.constants("dyros_bodies.h", "dwb_")
EXPORTS = list(cbind.signatures("dyros_bodies.h", "dwb_"))
DwbModel = cbind.structs("dyros_bodies.h", "dwb_")["DwbModel"]
NB, ROW, GROUP, TABLE_WORDS = K["DWB_NUM_BODIES"], K["DWB_ROW"], K["DWB_GROUP"], K["DWB_TABLE_WORDS"]
DEFAULTS = {"bodies": None, "com": True, "auto": False}


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_bodies.h", "dwb_")


def model_struct(model) -> DwbModel:
    """DwbModel from the compiled model (a TocabiModel or its dictionary)."""
    d = getattr(model, "d", model)
    m = DwbModel()

    def fill(field, values, dt):
        a = np.ascontiguousarray(values, dtype=dt)
        dst = getattr(m, field)
        if a.nbytes != C.sizeof(dst):
            raise ValueError("model key %r has %d bytes, DwbModel.%s holds %d" % (field, a.nbytes, field, C.sizeof(dst)))
        C.memmove(dst, a.ctypes.data, a.nbytes)
    for field in ("mv_parent", "body_moving", "inert_gym", "inert_mv"):
        fill(field, d[field], np.int32)
    for field in ("mv_pos", "mv_rot0", "mv_axis", "inert_mass", "inert_com"):
        fill(field, d[field], np.float32)
    return m


def pack_table(api: dict, model) -> np.ndarray:
    """The device table's DWB_TABLE_WORDS words as a uint32 array (dwb_pack_table; raises for a model it refuses)."""
    m, t = model if isinstance(model, DwbModel) else model_struct(model), np.zeros(TABLE_WORDS, np.uint32)
    cbind.check(api, api["pack_table"](C.byref(m), t.ctypes.data))
    return t


def body_ids(bodies, names) -> list:
    """Gym ids of a selection of names or ids (None: all, in order)."""
    if bodies is None:
        return list(range(len(names)))
    if isinstance(bodies, (str, bytes)) or not hasattr(bodies, "__len__") or not 1 <= len(bodies) <= NB:
        raise ValueError("body_states.bodies must be a list of 1..%d body names or Gym ids" % NB)
    out = []
    for b in bodies:
        if isinstance(b, str):
            if b not in names:
                raise ValueError("body_states.bodies: no body named %r" % (b,))
            out.append(list(names).index(b))
        elif isinstance(b, (int, np.integer)) and not isinstance(b, bool) and 0 <= int(b) < len(names):
            out.append(int(b))
        else:
            raise ValueError("body_states.bodies: %r is neither a body name nor a Gym id in 0..%d" % (b, len(names) - 1))
    return out


def resolve(spec, names=None) -> dict:
    """The cfg value as a full dict; None when the tensor is off (None or False).  ValueError for anything else that is not True or a dict of
    bodies / com / auto.  names: the model's body names (None: the packaged model's)."""
    out = resolve_front("body_states", spec, DEFAULTS, ("com", "auto"), "bodies, com and auto")
    if out is None:
        return None
    if names is None:
        from .model import load_model
        names = load_model().body_names
    out["ids"] = body_ids(out["bodies"], names)
    return out


def validate(spec) -> None:
    """Checks of cfg sim.mi355.body_states (config.validate_cfg)."""
    resolve(spec)


def select_parents(ids, body_parent) -> list:
    """The row of every selected body's Gym parent within the selection (its first occurrence), or -1."""
    first = {}
    for r, g in enumerate(ids):
        first.setdefault(g, r)
    return [first.get(body_parent[g], -1) if body_parent[g] >= 0 else -1 for g in ids]


class BodyStates(ModelTensor):
    """The rigid-body states of one env object's bound buffers (see the module docstring).  host: a DyrosDynamicWalk (TocabiAMPLower hands its
    physics host); vel_at_com: the host's root_vel_at_com unless given.  Buffers are allocated here, once."""

    WHAT = "tensor"

    def __init__(self, host, spec=True, vel_at_com=None):
        model = host.model
        spec = resolve(spec, model.body_names)
        super().__init__(host, spec, declare)
        N = self.num_envs
        self.ids = spec["ids"]
        self.names = [model.body_names[g] for g in self.ids]
        self.parents = select_parents(self.ids, model.body_parent)
        self.vel_at_com = self._vel_at_com(vel_at_com)
        self.dt = float(host.dt) * int(getattr(host, "skipframe", 1))
        self.table = self._upload(pack_table(self.api, model))
        nb = len(self.ids)
        self.states = self._zeros(N, nb, ROW)
        self.pos, self.rot = self.states[..., 0:3], self.states[..., 3:7]
        self.vel, self.ang_vel = self.states[..., 7:10], self.states[..., 10:13]
        self.com = self._zeros(N, K["DWB_COM_WORDS"]) if spec["com"] else None
        whole = self.ids == list(range(NB))
        self._ids_c = None if whole else (C.c_int32 * nb)(*self.ids)
        self._args = self._inputs() + (self._in("mass_scale", shape=(N, NB)), self._ids_c, 0 if whole else nb, self.vel_at_com,
                                       self.states.data_ptr(), ptr(self.com))

    def refresh(self):
        """One launch on torch's current stream; returns `states`."""
        self._launch("refresh", self._args)
        return self.states

    def index(self, name: str) -> int:
        """The row of a body (its first, where the selection repeats it)."""
        if name not in self.names:
            raise KeyError("body_states holds no body named %r" % (name,))
        return self.names.index(name)

    def rows(self, *names):
        """[N, len(names), 13]: the rows of the named bodies (a copy, in the order asked)."""
        return self.states[:, [self.index(n) for n in names]]
