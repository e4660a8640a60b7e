"""The foot force-torque sensors (include/dyros_sensors.h, csrc/dw_sensors.hip): Isaac Gym's
acquire_force_sensor_tensor / refresh_force_sensor_tensor for sensors on TOCABI's two feet, with the centre of pressure of each sole, the
whole-body ZMP and the eight sole corners beside it.

Opt-in: cfg["sim"]["mi355"]["force_sensors"] = True, or {"sensors": [{"body": "L_Foot_Link", "pos": [0, 0, -0.09], "quat": [0, 0, 0, 1],
"world_frame": False}, ...], "cop": True, "corners": False, "auto": False}, gives a DyrosDynamicWalk env a `force_sensors` attribute
(None otherwise; TocabiAMPLower: key `amp_force_sensors`).  refresh() makes one launch, dwf_refresh, on torch's current stream: the wrench
the ground exerts on each foot through the sole contact solve, from the per-corner impulses the solve keeps in the task record and the foot
pose that root_states and dof_state give.  It only reads the env's buffers, takes no argument that changes from call to call, allocates
nothing and does not synchronise, so it sits inside a captured rollout step.

    refresh()                 one launch; returns Gym's vec_sensor_tensor view [N, S * 6]
    sensors, force, torque    [N, S, 6] and its views [N, S, 3]: force then torque, in the sensor frame (world axes with "world_frame")
    cop, zmp                  [N, 2, 4]: x, y in the foot frame, Fz, loaded corners; [N, 4]: world x, y, total Fz, loaded corners (None with "cop": False)
    corners                   [N, 8, 6]: world position and force of every sole corner (None unless "corners": True)
    names, index(name)        the sensors' bodies

A sensor sits on L_Foot_Link / R_Foot_Link or on the jointless body welded to the same ankle link (Gym 7, 8, 15, 16).  Not measured: forces
on the foot that do not come from the sole solve (self-collision, penalty contacts of other primitives), gravity and joint forces; an env
that reset in the step reads zero.  Plane only: a cfg with height-field terrain is refused (the header says why).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import cbind
from .model_tensors import ModelTensor, ptr, resolve_front

K = cbind.constants("dyros_sensors.h", "dwf_")
EXPORTS = list(cbind.signatures("dyros_sensors.h", "dwf_"))
_S = cbind.structs("dyros_sensors.h", "dwf_")
DwfModel, DwfSensor = _S["DwfModel"], _S["DwfSensor"]
MAX_SENSORS, GROUP = K["DWF_MAX_SENSORS"], K["DWF_GROUP"]
DEFAULT_POS = (0.0, 0.0, -0.09)          # the reference's mount (tasks/dyros_dynamic_walk.py:303-313)
DEFAULTS = {"sensors": None, "cop": True, "corners": False, "auto": False}
SENSOR_DEFAULTS = {"body": None, "pos": DEFAULT_POS, "quat": (0.0, 0.0, 0.0, 1.0), "world_frame": False}
QUAT_TOL = 1e-3          # |norm - 1| a spec's quaternion may have; it is normalised here, in double


def declare(lib) -> dict:
    return cbind.declare(lib, "dyros_sensors.h", "dwf_")


def foot_bodies(model) -> dict:
    """Gym id -> foot (0 left, 1 right) of the bodies a sensor may sit on: the jointless bodies welded to the two feet's moving bodies."""
    d = getattr(model, "d", model)
    feet = [d["foot_pts"][0]["moving"], d["foot_pts"][4]["moving"]]
    return {g: feet.index(m) for g, m in enumerate(d["body_moving"]) if m in feet and g not in d["mv_gym"]}


def _vec(name, v, n):
    try:
        a = [float(x) for x in v]
    except (TypeError, ValueError):
        a = []
    if isinstance(v, (str, bytes)) or len(a) != n or not all(math.isfinite(x) for x in a):
        raise ValueError("force_sensors: %s must be %d finite numbers" % (name, n))
    return a


def resolve(spec, model=None, terrain=None) -> dict:
    """The cfg value as a full dict; None when the sensors are off (None or False).  ValueError for anything else that is not True or a dict
    of sensors / cop / corners / auto, for a sensor on another body than a foot's, more than 8 sensors, a quaternion that is not a unit
    one, and for terrain: a cfg["terrain"] whose mesh_type is a height field.  model: a TocabiModel (None: the packaged one)."""
    out = resolve_front("force_sensors", spec, DEFAULTS, ("cop", "corners", "auto"), "sensors, cop, corners and auto")
    if out is None:
        return None
    if dict(terrain or {}).get("mesh_type", "plane") in ("heightfield", "trimesh"):
        raise ValueError("force_sensors: plane only -- on a height field the task record holds the sole impulses in contact frames that "
                         "are not kept (include/dyros_sensors.h)")
    if model is None:
        from .model import load_model
        model = load_model()
    names, feet = list(model.body_names), foot_bodies(model)
    sens = out["sensors"]
    if sens is None:
        sens = [{"body": "L_Foot_Link"}, {"body": "R_Foot_Link"}]
    if isinstance(sens, (str, bytes, dict)) or not hasattr(sens, "__len__") or len(sens) > MAX_SENSORS:
        raise ValueError("force_sensors.sensors must be a list of at most %d sensor dicts" % MAX_SENSORS)
    full = []
    for s in sens:
        if not isinstance(s, dict) or set(s) - set(SENSOR_DEFAULTS) or "body" not in s:
            raise ValueError("force_sensors.sensors: a sensor is a dict with body and optionally pos, quat, world_frame; got %r" % (s,))
        s = dict(SENSOR_DEFAULTS, **s)
        b = s["body"]
        g = names.index(b) if isinstance(b, str) and b in names else (int(b) if isinstance(b, (int, np.integer)) and not isinstance(b, bool) else -1)
        if g not in feet:
            raise ValueError("force_sensors.sensors: body %r is not one of %s" % (b, [names[i] for i in sorted(feet)]))
        if not isinstance(s["world_frame"], bool):
            raise ValueError("force_sensors.sensors: world_frame must be True or False")
        q = _vec("quat", s["quat"], 4)
        n = math.sqrt(sum(x * x for x in q))
        if abs(n - 1.0) > QUAT_TOL:
            raise ValueError("force_sensors.sensors: quat %r is not a unit quaternion (xyzw)" % (s["quat"],))
        full.append({"body": names[g], "gym": g, "foot": feet[g], "pos": _vec("pos", s["pos"], 3), "quat": [x / n for x in q],
                     "world_frame": s["world_frame"]})
    if not full and not out["cop"] and not out["corners"]:
        raise ValueError("force_sensors: no sensor, no cop and no corners: nothing to compute")
    out["sensors"] = full
    return out


def validate(spec, terrain=None) -> None:
    """Checks of cfg sim.mi355.force_sensors (config.validate_cfg)."""
    resolve(spec, terrain=terrain)


def model_struct(model, dt) -> DwfModel:
    """DwfModel from the compiled model and the physics substep: inv_dt is formed as the step forms it, 1.0f / (float)dt."""
    d = getattr(model, "d", model)
    m = DwfModel()
    m.foot_mv[0], m.foot_mv[1] = d["foot_pts"][0]["moving"], d["foot_pts"][4]["moving"]
    for k, f in enumerate(d["foot_pts"]):
        if f["moving"] != m.foot_mv[k // 4]:
            raise ValueError("model: sole corners must be grouped 4 + 4")
        for i in range(3):
            m.foot_pos[k][i] = f["pos"][i]
    m.inv_dt = float(np.float32(1.0) / np.float32(dt))
    return m


def sensor_array(sensors):
    """(DwfSensor * S)() of resolved sensor dicts (None for none)."""
    if not sensors:
        return None
    arr = (DwfSensor * len(sensors))()
    for a, s in zip(arr, sensors):
        a.foot, a.world_frame = int(s["foot"]), int(bool(s["world_frame"]))
        for i in range(3):
            a.pos[i] = s["pos"][i]
        for i in range(4):
            a.quat[i] = s["quat"][i]
    return arr


class ForceSensors(ModelTensor):
    """The foot sensors of one env object's bound buffers (see the module docstring).  host: a DyrosDynamicWalk (TocabiAMPLower hands its
    physics host).  Buffers are allocated here, once."""

    WHAT = "sensors"

    def __init__(self, host, spec=True):
        from . import _lib
        from .body_states import declare as declare_bodies, pack_table
        model = host.model
        if getattr(host, "custom_origins", False):
            raise ValueError("force_sensors: plane only (include/dyros_sensors.h); this env runs on a height field")
        spec = resolve(spec, model)
        super().__init__(host, spec, declare)
        N = self.num_envs
        self.specs = spec["sensors"]
        self.names = [s["body"] for s in self.specs]
        self.dt = float(host.dt) * int(getattr(host, "skipframe", 1))
        self.table = self._upload(pack_table(declare_bodies(_lib.load()[0]), model))          # (dwb_pack_table's: the chain constants)
        self._model_c = model_struct(model, host.dt)
        self._sensors_c = sensor_array(self.specs)
        S = len(self.specs)
        self.sensors = self._zeros(N, S, K["DWF_SENSOR_WORDS"])
        self.force, self.torque = self.sensors[..., 0:3], self.sensors[..., 3:6]
        self.vec_sensor_tensor = self.sensors.view(N, S * K["DWF_SENSOR_WORDS"])
        self.cop = self._zeros(N, K["DWF_NUM_FEET"], K["DWF_COP_WORDS"]) if spec["cop"] else None
        self.zmp = self._zeros(N, K["DWF_ZMP_WORDS"]) if spec["cop"] else None
        self.corners = self._zeros(N, K["DWF_NUM_CORNERS"], K["DWF_CORNER_WORDS"]) if spec["corners"] else None
        self._args = self._inputs() + (self._in("env_state", shape=(N, K["DWF_ES_WORDS"])), C.byref(self._model_c), self._sensors_c, S,
                                       ptr(self.sensors) if S else None, ptr(self.cop), ptr(self.zmp), ptr(self.corners))

    def refresh(self):
        """One launch on torch's current stream; returns the [N, S * 6] view of `sensors`."""
        self._launch("refresh", self._args)
        return self.vec_sensor_tensor

    def index(self, name: str) -> int:
        """The first sensor on a body."""
        if name not in self.names:
            raise KeyError("force_sensors holds no sensor on %r" % (name,))
        return self.names.index(name)
