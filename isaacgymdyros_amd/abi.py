"""ctypes mirror of include/dyros_walk.h: the constants, the structs and the function prototypes are all read from the header (cbind.py).

The reference binds its native engine through pybind11 (`gym_3x.so`) and aliases sim-owned buffers
with `gymtorch.wrap_tensor` (reference: python/isaacgym/gymtorch.py:61-106).  Here buffers are
torch-owned and the native side only ever sees raw pointers, so plain ctypes is the whole binding.
"""
from __future__ import annotations

import ctypes as C
import os

from . import cbind

HEADER = os.path.join(cbind.INCLUDE, "dyros_walk.h")
K = cbind.constants("dyros_walk.h", "dw_")          # every integer #define of the header, e.g. K["DW_ES_WORDS"]
globals().update(K)
S = cbind.structs("dyros_walk.h", "dw_")            # every struct of the header as a ctypes.Structure, e.g. S["DwConfig"]
globals().update(S)
STRUCTS = tuple(S.values())
# the three pointer tables: device (or, for the oracle, host) pointers travel as plain addresses
BUFFER_NAMES = [n for n, _ in S["DwBuffers"]._fields_]
AMP_BUFFER_NAMES = [n for n, _ in S["DwAmpBuffers"]._fields_]             # the fused TocabiAMPLower step
AMP_RESET_DRAW_NAMES = [n for n, _ in S["DwAmpResetDraws"]._fields_]      # the caller's draws of dw_amp_reset_done, rows indexed by env
EXPORTS = list(cbind.signatures("dyros_walk.h", "dw_"))
# The fused TocabiAMPLower step (csrc/dw_amp_step.h) is carried by the HIP library and by the octet build of the host emulation
# (tests/emul/), its one-launch form and dw_amp_reset_ids by the HIP library alone; the C oracle has neither, nor dw_terrain_log.
_FUSED_AMP = ("amp_step_begin", "amp_step_mid", "amp_step_end", "amp_step", "amp_reset_rows", "amp_reset_done", "amp_reset_ids")
# the device-resident motion library (csrc/dw_amp_motion.h): the HIP library alone
_MOTION = ("amp_motion_state", "amp_motion_obs", "amp_reset_rows_motion", "amp_reset_done_motion")
MAY_LACK = {"dw_": (),
            "dwo_": _FUSED_AMP + _MOTION + ("terrain_log",),
            "dwe_": _FUSED_AMP + _MOTION + ("step_obs", "amp_observations", "amp_disc_observations", "amp_reward", "amp_reset", "newwalk_reward",
                                  "body_positions")}


def declare(lib: C.CDLL, prefix: str = "dw_"):
    """Every entry point bound with the types its prototype in the header has (cbind); raises AttributeError if the shared object lacks one of
    them that a library of this prefix has to export, DyrosWalkLibraryError if its ABI version is not the header's."""
    return cbind.declare(lib, "dyros_walk.h", "dw_", symbols=prefix, may_lack=MAY_LACK[prefix])


# name -> (per-env shape, numpy dtype string); gate_acc is the one buffer without an env dimension
BUFFER_SPECS = {
    "root_states": ((13,), "f4"),
    "dof_state": ((K["DW_NUM_DOF"], 2), "f4"),
    "contact_forces": ((K["DW_NUM_BODIES"], 3), "f4"),
    "mass_scale": ((K["DW_NUM_BODIES"],), "f4"),
    "dof_damping": ((K["DW_NUM_DOF"],), "f4"),
    "dof_armature": ((K["DW_NUM_DOF"],), "f4"),
    "friction_scale": ((), "f4"),
    "total_mass": ((), "f4"),
    "env_origins": ((3,), "f4"),
    "obs_buf": ((K["DW_NUM_OBS"],), "f4"),
    "rew_buf": ((), "f4"),
    "reset_buf": ((), "i8"),
    "progress_buf": ((), "i8"),
    "timeout_buf": ((), "i8"),
    "randomize_buf": ((), "i8"),
    "stacked_rewards": ((K["DW_NUM_REW"],), "f4"),
    "env_state": ((K["DW_ES_WORDS"],), "f4"),
    "obs_history": ((K["DW_HIST_SLOTS"], K["DW_NUM_OBS1"]), "f4"),
    "action_history": ((K["DW_HIST_SLOTS"], K["DW_NUM_ACT"]), "f4"),
    "gate_acc": (None, "i8"),
    # terrain (row f-4): two tables shared by all envs (one-element placeholders on the ground plane) and two per-env words
    "height_samples": (None, "i2"),
    "terrain_origins": (None, "f4"),
    "terrain_levels": ((), "i8"),
    "terrain_types": ((), "i8"),
}
GATE_ACC_WORDS = K["DW_GATE_WORDS"]
# element counts of the buffers that are not per-env (shape None above); the terrain tables are re-allocated by the
# host class when a height field is configured
GLOBAL_WORDS = {"gate_acc": GATE_ACC_WORDS, "height_samples": 4, "terrain_origins": 3}

# env-state record fields: name -> (word offset, shape, 'f' float32 | 'i' int32); see DW_ES_* in the header
ES_FIELDS = {
    "qpos_noise": (K["DW_ES_QPOS_NOISE"], (33,), "f"),
    "qvel_noise": (K["DW_ES_QVEL_NOISE"], (33,), "f"),
    "qpos_pre": (K["DW_ES_QPOS_PRE"], (33,), "f"),
    "pre_joint_velocity_states": (K["DW_ES_PRE_QVEL"], (33,), "f"),
    "target_data_qpos": (K["DW_ES_TARGET_QPOS"], (33,), "f"),
    "target_data_force": (K["DW_ES_TARGET_FORCE"], (2,), "f"),
    "target_vel": (K["DW_ES_TARGET_VEL"], (2,), "f"),
    "motor_constant_scale": (K["DW_ES_MOTOR_SCALE"], (12,), "f"),
    "qpos_bias": (K["DW_ES_QPOS_BIAS"], (12,), "f"),
    "quat_bias": (K["DW_ES_QUAT_BIAS"], (3,), "f"),
    "action_log": (K["DW_ES_ACTION_LOG"], (6, 12), "f"),
    "actions": (K["DW_ES_ACTIONS"], (13,), "f"),
    "actions_pre": (K["DW_ES_ACTIONS_PRE"], (13,), "f"),
    "action_torque": (K["DW_ES_ACTION_TORQUE"], (12,), "f"),
    "action_torque_pre": (K["DW_ES_ACTION_TORQUE_PRE"], (12,), "f"),
    "foot_force_pre": (K["DW_ES_FOOT_FORCE_PRE"], (2, 3), "f"),
    "time": (K["DW_ES_TIME"], (1,), "f"),
    "epi_len": (K["DW_ES_EPI_LEN"], (), "f"),
    "epi_len_log": (K["DW_ES_EPI_LEN_LOG"], (), "f"),
    "contact_reward_sum": (K["DW_ES_CRS"], (), "f"),
    "contact_reward_mean": (K["DW_ES_CRM"], (), "f"),
    "magnitude": (K["DW_ES_MAGNITUDE"], (), "f"),
    "phase": (K["DW_ES_PHASE"], (), "f"),
    "init_mocap_data_idx": (K["DW_ES_INIT_MOCAP"], (1,), "i"),
    "mocap_data_idx": (K["DW_ES_MOCAP_IDX"], (1,), "i"),
    "delay_idx": (K["DW_ES_DELAY_IDX"], (), "i"),
    "simul_len": (K["DW_ES_SIMUL_LEN"], (), "i"),
    "perturbation_count": (K["DW_ES_PERT_COUNT"], (), "i"),
    "pert_duration": (K["DW_ES_PERT_DURATION"], (), "i"),
    "pert_on": (K["DW_ES_PERT_ON"], (), "i"),
    "impulse": (K["DW_ES_IMPULSE"], (), "i"),
    "perturb_timing": (K["DW_ES_PERT_TIMING"], (), "i"),
    "perturb_start": (K["DW_ES_PERT_START"], (1,), "i"),
    "hist_head": (K["DW_ES_HIST_HEAD"], (), "i"),
    "nan_resets": (K["DW_ES_NAN_RESETS"], (), "i"),
    "warm_impulses": (K["DW_ES_WARM"], (8, 3), "f"),
    "episode_return": (K["DW_ES_EPI_RETURN"], (), "f"),
    "last_episode_return": (K["DW_ES_LAST_RETURN"], (), "f"),
    "episodes_finished": (K["DW_ES_EPISODES"], (), "i"),
}


def es_view(env_state, name):
    """View of one named field of the [N, DW_ES_WORDS] record array (numpy array or torch tensor)."""
    off, shape, kind = ES_FIELDS[name]
    n = 1
    for s in shape:
        n *= s
    v = env_state[:, off:off + n]
    if kind == "i":
        v = v.view(_int32_of(env_state))
    return v.reshape((env_state.shape[0],) + tuple(shape))


def _int32_of(arr):
    try:
        import torch
        if isinstance(arr, torch.Tensor):
            return torch.int32
    except ImportError:
        pass
    import numpy as np
    return np.int32
