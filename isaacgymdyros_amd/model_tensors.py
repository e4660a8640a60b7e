"""What the model-tensor features share on the host (DESIGN.md sections 21-30): the tables of the features, FEATURES, SOLVERS and SENSORS, by which the env classes
and config.validate_cfg validate, attach and refresh them; the common front of their resolve(); and ModelTensor, the base of their classes.

A feature is a module of this package with K, EXPORTS, DEFAULTS, declare, resolve and validate, and a class over one env object's bound
buffers with `auto` and refresh().  DyrosDynamicWalk reads cfg sim.mi355.<name> and TocabiAMPLower sim.mi355.amp_<name> (its own keys: the
plain ones would reach its physics host, a DyrosDynamicWalk); either gets an attribute <name>: the object, or None when the key is absent or
False: no buffer then, and step() makes no extra launch.
"""
from __future__ import annotations

import importlib

from . import cbind

# (name: module, env attribute and cfg key; class; the top-level cfg keys whose values validate() takes after the spec), in cfg order
FEATURES = (
    ("body_states", "BodyStates", ()),                     # the rigid-body state tensor [N, K, 13] and the centre of mass
    ("force_sensors", "ForceSensors", ("terrain",)),       # the foot force-torque sensors [N, S, 6], the soles' centres of pressure, the ZMP; plane only
    ("jacobians", "Jacobians", ()),                        # the Jacobian tensor [N, K, 6, 39], the mass matrix [N, 39, 39], the COM Jacobian
    ("dynamics", "Dynamics", ()),                          # the bias-force, gravity, inverse-dynamics and momentum tensors [N, 39] / [N, 6]
    ("forward_dynamics", "ForwardDynamics", ()),           # the solve of M nu_dot = rhs - h, the factor M = L' D L and M^-1
    ("contact_dynamics", "ContactDynamics", ()),           # the same under rigid contacts: J_c, the contact-space inertia, accelerations and forces
    ("contact_inverse_dynamics", "ContactInverseDynamics", ()),   # the inverse question: the joint torques and contact wrenches of a wanted acceleration
    ("stance_inverse_dynamics", "StanceInverseDynamics", ("terrain",)),   # the same per env's stance, with the soles' feasibility margins; plane only
)
# FEATURES holds the tensors of the state the simulator is in.  SOLVERS holds what asks the opposite question -- which state would do -- and is
# walked after it: validated, attached and refreshed the same way, under the same keys
SOLVERS = (
    ("inverse_kinematics", "InverseKinematics", ()),       # the joint angles (and base pose) that put bodies at wanted poses [N, 33]
)


# SENSORS holds what looks at the world around the robot rather than at the robot, walked last
SENSORS = (
    ("height_scan", "HeightScan", ("terrain",)),           # the ground's heights at a yaw-aligned grid around the base [N, P], the soles' clearance [N, B]
)


def _all():
    return FEATURES + SOLVERS + SENSORS


def _module(name):
    return importlib.import_module("." + name, __package__)


def validate_all(cfg: dict, prefix: str = "") -> None:
    """Every feature's validate() of cfg sim.mi355.<prefix><name>: ValueError before anything is loaded or allocated."""
    mi = cfg["sim"].get("mi355", {})
    for name, _, extra in _all():
        if mi.get(prefix + name) is not None:
            _module(name).validate(mi[prefix + name], *(cfg.get(k) for k in extra))


def attach(env, host, mi355: dict, prefix: str = "") -> None:
    """env.<name> of every feature: its object over host's bound buffers where mi355[<prefix><name>] switches it on, None otherwise."""
    for name, cls, _ in _all():
        spec = mi355.get(prefix + name)
        on = spec is not None and spec is not False          # (as validate reads it: {} is the default spec)
        f = getattr(_module(name), cls)(host, spec) if on else None
        if f is not None:
            f.task_host = host is env          # (a feature that reads task state asks whether the physics host's task is the env's)
        setattr(env, name, f)


def refresh_auto(env) -> None:
    """refresh() of every attached feature with "auto": True, in cfg order (after step(), reset_idx() and reset())."""
    for name, _, _ in _all():
        f = getattr(env, name)
        if f is not None and f.auto:
            f.refresh()


def resolve_front(name: str, spec, defaults: dict, bools, keys: str = None) -> dict:
    """The front of a feature's resolve(): None when the cfg value switches the feature off (None or False), else the defaults overlaid with
    the spec (True: the defaults).  ValueError for a value that is neither, for unknown keys and for a key of `bools` that is not a bool.
    keys: how the first message lists the keys (the defaults' keys, unless given)."""
    if spec is None or spec is False:
        return None
    if spec is True:
        spec = {}
    if not isinstance(spec, dict):
        raise ValueError("%s must be True, False or a dict with %s" % (name, keys or ", ".join(defaults)))
    unknown = set(spec) - set(defaults)
    if unknown:
        raise ValueError("%s: unknown keys %s" % (name, sorted(unknown, key=str)))
    out = dict(defaults, **spec)
    for k in bools:
        if not isinstance(out[k], bool):
            raise ValueError("%s.%s must be True or False" % (name, k))
    return out


def ptr(t):
    return None if t is None else t.data_ptr()


def joint_space_force(r, tau_joint=None, gen_force=None):
    """r [N, 39] = [0; tau_joint] + gen_force in place: tau_joint [N, 33] and gen_force [N, 39], each or None (zero)."""
    if gen_force is not None:
        r.copy_(gen_force)
    else:
        r.zero_()
    if tau_joint is not None:
        r[:, 6:] += tau_joint


class ModelTensor(cbind.Launcher):
    """The base of the features' classes: the entry points, the host's bound buffers as checked pointers, and the launch.  A subclass is its
    buffers, its argument tuples (built once: the host's buffers are bound once, so no argument changes from call to call) and its methods."""

    WHAT = "tensors"          # in the ValueError for a spec that switches the feature off

    def __init__(self, host, spec, declare):
        """spec: what the module's resolve() made of the cfg value; declare: the module's."""
        from . import _lib
        if spec is None:
            raise ValueError("%s: the spec switches the %s off" % (type(self).__name__, self.WHAT))
        self.api = declare(_lib.load()[0])
        self.host = host
        self.num_envs, self._tdev, self.auto = host.num_envs, host._tdev, spec["auto"]

    def _vel_at_com(self, vel_at_com) -> int:
        return int(bool(self.host._ccfg.root_vel_at_com if vel_at_com is None else vel_at_com))

    def _upload(self, table):
        """A packed table (uint32 words) on the device."""
        import numpy as np
        import torch
        return torch.from_numpy(table.view(np.int32)).to(self._tdev)

    def _zeros(self, *shape):
        import torch
        return torch.zeros(*shape, dtype=torch.float32, device=self._tdev)

    def _in(self, name, **kw) -> int:
        """The pointer of one of the host's float32 buffers, its shape or size checked."""
        import torch
        from .ppo_update import _req
        return _req(name, self.host._buf[name], torch.float32, **kw).data_ptr()

    def _inputs(self, armature=None) -> tuple:
        """The arguments every entry point begins with: num_envs, `table`, root_states, dof_state; with armature given (the spec's bool) also
        mass_scale and dof_armature (None where armature is False)."""
        from .jacobians import K, NB
        N = self.num_envs
        a = (N, self.table.data_ptr(), self._in("root_states", shape=(N, 13)), self._in("dof_state", numel=N * 66))
        if armature is None:
            return a
        return a + (self._in("mass_scale", shape=(N, NB)), self._in("dof_armature", shape=(N, K["DWJ_NUM_DOF"])) if armature else None)
