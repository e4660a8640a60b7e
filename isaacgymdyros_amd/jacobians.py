"""The Jacobian and mass-matrix tensors (include/dyros_jacobians.h, csrc/dw_jacobian.hip): Isaac Gym's
acquire_jacobian_tensor / refresh_jacobian_tensors and acquire_mass_matrix_tensor / refresh_mass_matrix_tensors for TOCABI, computed on the GPU.

Opt-in: cfg["sim"]["mi355"]["jacobians"] = True, or {"bodies": [names or Gym ids], "jacobian": True, "mass_matrix": True, "com_jacobian": False,
"armature": True, "auto": False}, gives a DyrosDynamicWalk env a `jacobians` attribute (None otherwise; TocabiAMPLower: key `amp_jacobians`).
Each refresh is one launch on torch's current stream.  It only reads the env's buffers, takes no argument that changes from call to call,
allocates nothing and does not synchronise, so it sits inside a captured rollout step.

The generalised velocity is nu = [root_states[:, 7:10], root_states[:, 10:13], dof_vel], 39 numbers in world axes; DoF j is column 6 + j.

    refresh_jacobian()        one launch (dwj_jacobian); returns `jacobian` [N, K, 6, 39]: rows 0:3 linear, 3:6 angular;
                              jacobian[e, r] @ nu[e] = body_states' words [7:13] of the same body (its COM's velocity with root_vel_at_com)
    refresh_mass_matrix()     one launch (dwj_mass_matrix); returns `mass_matrix` [N, 39, 39], symmetric bit for bit; fills `com_jacobian` too
    refresh()                 both
    mm                        the view mass_matrix[:, 6:, 6:]: Gym's (num_dofs, num_dofs) matrix
    com_jacobian              [N, 3, 39] = mass_matrix[:, 0:3] / total mass: com_jacobian @ nu = the COM's velocity (None unless asked for)
    names, ids, dof_names     of the K rows and the 33 DoF columns
    dof_mask                  [K, 39] bool: the columns of a row that can be non-zero (every other word is +0.0)
    index(name), rows(*names)

"armature": True adds the env's dof_armature to the joints' diagonal.  "auto": True refreshes after every step(), after reset_idx() and reset().
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import cbind
from .body_states import body_ids
from .model_tensors import ModelTensor, ptr, resolve_front

K = cbind.constants("dyros_jacobians.h", "dwj_")
EXPORTS = list(cbind.signatures("dyros_jacobians.h", "dwj_"))
DwjModel = cbind.structs("dyros_jacobians.h", "dwj_")["DwjModel"]
NB, NM, NV, GROUP, TABLE_WORDS = K["DWJ_NUM_BODIES"], K["DWJ_NUM_MOVING"], K["DWJ_NV"], K["DWJ_GROUP"], K["DWJ_TABLE_WORDS"]
DEFAULTS = {"bodies": None, "jacobian": True, "mass_matrix": True, "com_jacobian": False, "armature": True, "auto": False}


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_jacobians.h", "dwj_")


def model_struct(model) -> DwjModel:
    """DwjModel from the compiled model (a TocabiModel or its dictionary)."""
    d = getattr(model, "d", model)
    m = DwjModel()

    def fill(field, values, dt):
        a = np.ascontiguousarray(values, dtype=dt)
        dst = getattr(m, field)
        if a.nbytes != C.sizeof(dst):
            raise ValueError("model key %r has %d bytes, DwjModel.%s holds %d" % (field, a.nbytes, field, C.sizeof(dst)))
        C.memmove(dst, a.ctypes.data, a.nbytes)
    for field in ("mv_parent", "body_moving", "inert_gym", "inert_mv"):
        fill(field, d[field], np.int32)
    for field in ("mv_pos", "mv_rot0", "mv_axis", "inert_mass", "inert_com"):
        fill(field, d[field], np.float32)
    I = np.asarray(d["inert_I"], np.float64)
    if I.shape != (K["DWJ_NUM_INERT"], 3, 3):
        raise ValueError("model key 'inert_I' has shape %s, not (36, 3, 3)" % (I.shape,))
    fill("inert_I", np.stack([I[:, 0, 0], I[:, 1, 1], I[:, 2, 2], I[:, 0, 1], I[:, 0, 2], I[:, 1, 2]], 1), np.float32)
    return m


def pack_table(api: dict, model, words: int = TABLE_WORDS) -> np.ndarray:
    """The device table's DWJ_TABLE_WORDS words as a uint32 array (dwj_pack_table; raises for a model it refuses).  words: the table's size
    where api is another ABI's whose table begins with this one (dynamics.py, forward_dynamics.py)."""
    m, t = model if isinstance(model, DwjModel) else model_struct(model), np.zeros(words, np.uint32)
    cbind.check(api, api["pack_table"](C.byref(m), t.ctypes.data))
    return t


def resolve(spec, names=None) -> dict:
    """The cfg value as a full dict; None when the tensors are off (None or False).  ValueError for anything else that is not True or a dict of
    the keys of DEFAULTS.  names: the model's body names (None: the packaged model's)."""
    out = resolve_front("jacobians", spec, DEFAULTS, ("jacobian", "mass_matrix", "com_jacobian", "armature", "auto"))
    if out is None:
        return None
    if not out["jacobian"] and not out["mass_matrix"]:
        raise ValueError("jacobians: neither jacobian nor mass_matrix: nothing to compute")
    if out["com_jacobian"] and not out["mass_matrix"]:
        raise ValueError("jacobians.com_jacobian is a by-product of mass_matrix: set mass_matrix too")
    if names is None:
        from .model import load_model
        names = load_model().body_names
    try:
        out["ids"] = body_ids(out["bodies"], names)
    except ValueError as e:
        raise ValueError(str(e).replace("body_states.", "jacobians.")) from None
    return out


def validate(spec) -> None:
    """Checks of cfg sim.mi355.jacobians (config.validate_cfg)."""
    resolve(spec)


def dof_mask(ids, model) -> np.ndarray:
    """[K, 39] bool: columns 0:6, and column 6 + j where moving body j + 1 is the row's carrier or one of its ancestors."""
    d = getattr(model, "d", model)
    m = np.zeros((len(ids), NV), bool)
    m[:, 0:6] = True
    for r, g in enumerate(ids):
        b = d["body_moving"][g]
        while b > 0:
            m[r, 5 + b] = True
            b = d["mv_parent"][b]
    return m


class Jacobians(ModelTensor):
    """The Jacobians and the mass matrix of one env object's bound buffers (see the module docstring).  host: a DyrosDynamicWalk (TocabiAMPLower
    hands its physics host); vel_at_com: the host's root_vel_at_com unless given.  Buffers are allocated here, once."""

    def __init__(self, host, spec=True, vel_at_com=None):
        import torch
        model = host.model
        spec = resolve(spec, model.body_names)
        super().__init__(host, spec, declare)
        N = self.num_envs
        self.ids = spec["ids"]
        self.names = [model.body_names[g] for g in self.ids]
        self.dof_names = list(model.dof_names)
        self.dof_mask = torch.from_numpy(dof_mask(self.ids, model)).to(self._tdev)
        self.vel_at_com = self._vel_at_com(vel_at_com)
        self.dt = float(host.dt) * int(getattr(host, "skipframe", 1))
        self.table = self._upload(pack_table(self.api, model))
        nb = len(self.ids)
        self.jacobian = self._zeros(N, nb, K["DWJ_JAC_ROWS"], NV) if spec["jacobian"] else None
        self.mass_matrix = self._zeros(N, NV, NV) if spec["mass_matrix"] else None
        self.mm = None if self.mass_matrix is None else self.mass_matrix[:, 6:, 6:]
        self.com_jacobian = self._zeros(N, 3, NV) if spec["com_jacobian"] else None
        whole = self.ids == list(range(NB))
        self._ids_c = None if whole else (C.c_int32 * nb)(*self.ids)
        self._jac_args = None if self.jacobian is None else self._inputs() + (self._ids_c, 0 if whole else nb, self.vel_at_com, self.jacobian.data_ptr())
        self._mm_args = None if self.mass_matrix is None else self._inputs(spec["armature"]) + (self.vel_at_com, self.mass_matrix.data_ptr(),
                                                                                                ptr(self.com_jacobian))

    def refresh_jacobian(self):
        """One launch on torch's current stream; returns `jacobian`."""
        if self._jac_args is None:
            raise RuntimeError("jacobians: the Jacobian is switched off (cfg sim.mi355.jacobians: jacobian)")
        self._launch("jacobian", self._jac_args)
        return self.jacobian

    def refresh_mass_matrix(self):
        """One launch on torch's current stream; returns `mass_matrix` (and fills `com_jacobian`)."""
        if self._mm_args is None:
            raise RuntimeError("jacobians: the mass matrix is switched off (cfg sim.mi355.jacobians: mass_matrix)")
        self._launch("mass_matrix", self._mm_args)
        return self.mass_matrix

    def refresh(self):
        """Every tensor the spec holds: one launch each."""
        if self._jac_args is not None:
            self.refresh_jacobian()
        if self._mm_args is not None:
            self.refresh_mass_matrix()

    def index(self, name: str) -> int:
        """The row of a body (its first, where the selection repeats it)."""
        if name not in self.names:
            raise KeyError("jacobians holds no body named %r" % (name,))
        return self.names.index(name)

    def rows(self, *names):
        """[N, len(names), 6, 39]: the Jacobians of the named bodies (a copy, in the order asked)."""
        if self.jacobian is None:
            raise RuntimeError("jacobians: the Jacobian is switched off (cfg sim.mi355.jacobians: jacobian)")
        return self.jacobian[:, [self.index(n) for n in names]]
