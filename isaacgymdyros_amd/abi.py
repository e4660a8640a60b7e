"""ctypes mirror of include/dyros_walk.h: the structs by hand; the constants and the function prototypes are read from the header (cbind.py).

The reference binds its native engine through pybind11 (`gym_3x.so`) and aliases sim-owned buffers
with `gymtorch.wrap_tensor` (reference: python/isaacgym/gymtorch.py:61-106).  Here buffers are
torch-owned and the native side only ever sees raw pointers, so plain ctypes is the whole binding.
"""
from __future__ import annotations

import ctypes as C
import os

from . import cbind
from .model import DwModel, DwGeom  # noqa: F401  (re-exported)

HEADER = os.path.join(cbind.INCLUDE, "dyros_walk.h")
K = cbind.constants("dyros_walk.h", "dw_")          # every integer #define of the header, e.g. K["DW_ES_WORDS"]
globals().update(K)


class DwTaskConst(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_float)) for n in
                ("kp", "kv", "action_high", "initial_dof_pos", "mocap", "obs_mean", "obs_var",
                 "dof_armature_nominal", "dof_damping_nominal")]


class DwConfig(C.Structure):
    _fields_ = [
        ("dt", C.c_double),
        ("num_envs", C.c_int32),
        ("control_freq_inv", C.c_int32),
        ("gravity", C.c_float * 3),
        ("solver_iterations", C.c_int32),
        ("contact_offset", C.c_float),
        ("max_depenetration_velocity", C.c_float),
        ("friction", C.c_float),
        ("erp", C.c_float),
        ("contact_cfm", C.c_float),
        ("penalty_stiffness", C.c_float),
        ("penalty_damping", C.c_float),
        ("max_angular_velocity", C.c_float),
        ("max_episode_length", C.c_float),
        ("initial_height", C.c_float),
        ("death_cost", C.c_float),
        ("perturb", C.c_int32),
        ("force_perturb_start", C.c_int32),
        ("randomize_dof_on_reset", C.c_int32),
        ("dr_damping_add", C.c_float * 2),
        ("dr_armature_scale", C.c_float * 2),
        ("randomize_friction_on_reset", C.c_int32),
        ("dr_friction_scale", C.c_float * 2),
        ("timeout_fix", C.c_int32),
        ("root_vel_at_com", C.c_int32),
        ("torch_gpu_div", C.c_int32),
        ("self_collision", C.c_int32),
        ("debug_freeze_physics", C.c_int32),
        ("seed", C.c_uint64),
        ("terrain", C.c_int32),
        ("terrain_rows", C.c_int32),
        ("terrain_cols", C.c_int32),
        ("terrain_hscale", C.c_float),
        ("terrain_vscale", C.c_float),
        ("terrain_border", C.c_float),
        ("terrain_curriculum", C.c_int32),
        ("terrain_num_levels", C.c_int32),
        ("terrain_num_types", C.c_int32),
        ("terrain_env_length", C.c_float),
        ("max_episode_length_s", C.c_float),
        ("custom_origins", C.c_int32),
        ("pipeline", C.c_int32),
        ("debug_wave_build", C.c_int32),
    ]


_F = C.c_void_p   # device (or, for the oracle, host) pointers travel as plain addresses


class DwBuffers(C.Structure):
    _fields_ = [(n, _F) for n in (
        "root_states", "dof_state", "contact_forces",
        "mass_scale", "dof_damping", "dof_armature", "friction_scale", "total_mass", "env_origins",
        "obs_buf", "rew_buf", "reset_buf", "progress_buf", "timeout_buf", "randomize_buf",
        "stacked_rewards", "env_state", "obs_history", "action_history", "gate_acc",
        "height_samples", "terrain_origins", "terrain_levels", "terrain_types")]


BUFFER_NAMES = [n for n, _ in DwBuffers._fields_]


AMP_BUFFER_NAMES = ["actions", "actions_pre", "action_history", "obs_history", "commands", "start_target_vel", "final_target_vel",
                    "vel_change_duration", "cur_vel_change_duration", "epi_len", "power_scale", "action_log", "delay_idx", "simul_len",
                    "qpos_noise", "qvel_noise", "qpos_pre", "qpos_bias", "quat_bias", "dof_vel_pre", "tau", "progress_buf", "randomize_buf",
                    "reset_buf", "terminate_buf", "timeout_buf", "rigid_body_pos", "rigid_body_rot", "foot_pos", "obs1", "obs_buf", "obs_out",
                    "rew_buf", "reward_values", "total_mass", "amp_obs_buf", "amp_obs1", "motor_efforts", "p_gains", "d_gains", "init_angle",
                    "pd_action_offset", "pd_action_scale", "epi_len_log", "perturbation_count", "perturb_timing", "pert_on", "initial_root_states",
                    "hist_head", "draw_ctr", "nominal_damping", "nominal_armature"]


class DwAmpBuffers(C.Structure):            # include/dyros_walk.h, the fused TocabiAMPLower step
    _fields_ = [(n, C.c_void_p) for n in AMP_BUFFER_NAMES]


class DwAmpConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_envs", "num_his", "num_skip", "log_slots", "amp_steps", "pd_control", "noise", "vel_change",
                                         "local_root_obs", "enable_early_termination")] + \
               [(n, C.c_float) for n in ("clip_actions", "clip_obs", "max_episode_length", "termination_height", "inv_dt", "dt")] + \
               [("gpu_div", C.c_int32), ("cmd_lo", C.c_float * 3), ("cmd_scale", C.c_float * 3)] + \
               [(n, C.c_int32) for n in ("hist_ring", "device_draws", "randomize", "dr_damping", "dr_armature", "dr_frequency")] + \
               [("dr_damping_range", C.c_float * 2), ("dr_armature_range", C.c_float * 2), ("delay_idx_range", C.c_int32 * 2), ("seed", C.c_uint64)]


AMP_RESET_DRAW_NAMES = ["power_scale_u", "rootvel_noise", "cmd_x_u", "cmd_y_u", "cmd_yaw_u", "qpos_bias_u", "quat_bias_u", "damping_u", "armature_u",
                        "perturb_timing", "delay_idx"]


class DwAmpResetDraws(C.Structure):         # include/dyros_walk.h: the caller's draws of dw_amp_reset_done, rows indexed by env
    _fields_ = [(n, C.c_void_p) for n in AMP_RESET_DRAW_NAMES]


STRUCTS = (DwConfig, DwModel, DwTaskConst, DwBuffers, DwAmpBuffers, DwAmpConfig, DwAmpResetDraws)
EXPORTS = list(cbind.signatures("dyros_walk.h", "dw_", STRUCTS))
# The fused TocabiAMPLower step (csrc/dw_amp_step.h) is carried by the HIP library and by the octet build of the host emulation
# (tests/emul/), its one-launch form and dw_amp_reset_ids by the HIP library alone; the C oracle has neither, nor dw_terrain_log.
_FUSED_AMP = ("amp_step_begin", "amp_step_mid", "amp_step_end", "amp_step", "amp_reset_rows", "amp_reset_done", "amp_reset_ids")
MAY_LACK = {"dw_": (),
            "dwo_": _FUSED_AMP + ("terrain_log",),
            "dwe_": _FUSED_AMP + ("step_obs", "amp_observations", "amp_disc_observations", "amp_reward", "amp_reset", "newwalk_reward",
                                  "body_positions")}


def declare(lib: C.CDLL, prefix: str = "dw_"):
    """Every entry point bound with the types its prototype in the header has (cbind); raises AttributeError if the shared object lacks one of
    them that a library of this prefix has to export, DyrosWalkLibraryError if its ABI version is not the header's."""
    return cbind.declare(lib, "dyros_walk.h", "dw_", STRUCTS, symbols=prefix, may_lack=MAY_LACK[prefix])


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
