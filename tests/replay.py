"""Replay of the committed golden fixtures through a backend (CPU oracle or HIP library).  Test helper."""
import os

import numpy as np

from isaacgymdyros_amd import abi
from oracle import parity as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fields that involve no transcendental and no physics: must match the reference bit for bit
EXACT_LOGIC = ["reset_buf", "progress_buf", "timeout_buf", "delay_idx", "simul_len", "init_mocap_data_idx",
               "mocap_data_idx", "perturbation_count", "pert_on", "perturb_timing", "action_torque",
               "target_data_qpos", "target_data_force", "time", "epi_len", "epi_len_log", "motor_constant_scale",
               "qpos_bias", "quat_bias", "target_vel", "contact_reward_sum", "contact_reward_mean"]
# exp / sin / cos / asin / atan2 sit between these and their inputs: glibc (oracle), SLEEF (torch CPU, the
# goldens) and OCML (GPU) each round the last bit their own way
TRANSCENDENTAL = {"rew_buf": (1e-6, 2e-6), "stacked_rewards": (1e-6, 2e-6), "obs_buf": (2e-6, 4e-6),
                  "magnitude": (0.0, 0.0), "phase": (0.0, 0.0)}


class GoldenTerrain:
    """The height field of a terrain fixture, with the attributes OracleSim(terrain=...) reads."""

    def __init__(self, g):
        import types
        rows, cols = int(g["cfg_terrain_rows"]), int(g["cfg_terrain_cols"])
        lv, ty = int(g["cfg_terrain_num_levels"]), int(g["cfg_terrain_num_types"])
        self.heightsamples = g["init_height_samples"].reshape(rows, cols)
        self.env_origins = g["init_terrain_origins"].reshape(lv, ty, 3)
        self.tot_rows, self.tot_cols = rows, cols
        self.env_length = float(g["cfg_terrain_env_length"])
        self.cfg = types.SimpleNamespace(horizontal_scale=float(g["cfg_terrain_hscale"]), vertical_scale=float(g["cfg_terrain_vscale"]),
                                         border_size=float(g["cfg_terrain_border"]), curriculum=bool(g["cfg_terrain_curriculum"]),
                                         num_rows=lv, num_cols=ty)


def load(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: z[k] for k in z.files}


def golden_cfg(g, *names):
    """DwConfig overrides a fixture records as cfg_<field> (task_logic_altcfg.npz: the values the reference ran with)."""
    names = names or [k[4:] for k in g if k.startswith("cfg_")]
    return {k: float(g["cfg_" + k]) for k in names}


class OracleBackend:
    def __init__(self, N, task_const, **cfg):
        from oracle.oracle import OracleSim
        self.sim = OracleSim(N, task_const=task_const, **cfg)

    def load_buffers(self, bufs):
        for k, v in bufs.items():
            self.sim.buf[k][...] = v

    def write_state(self, root, dof, cf):
        self.sim.buf["root_states"][...] = root
        self.sim.buf["dof_state"][...] = dof
        self.sim.buf["contact_forces"][...] = cf

    def step(self, a, nz, t):
        self.sim.step(a, nz, t)

    def read_buffers(self):
        return self.sim.buf


class SimBackend(OracleBackend):
    """The replay interface over any driver with OracleSim's buf / step (EmulSim, the GPU tests' HipSim)."""

    def __init__(self, sim):
        self.sim = sim


# DwConfig sets of the task logic that the reference has no counterpart for (or that its fixtures do not move), each with the
# knob it is about: what the set reverts to the default for its baseline run, and the recorded fields that knob must change.
# max_episode_length = 7993 puts the two counters task_logic_frozen.npz injects (7990, 7996) at the time-out.
TASK_KNOB_SETS = {
    "timeout_fix": (dict(timeout_fix=1, death_cost=-1.5, max_episode_length=7993.0, initial_height=0.97),
                    dict(timeout_fix=0), ["timeout_buf"]),
    # (root_vel_at_com rides along: the physics alone reads it, so with physics frozen it owns no field here -- the case
    #  root_vel_at_origin of tests/knob_cases.py holds it)
    "perturb_off": (dict(perturb=0, root_vel_at_com=0, death_cost=-0.75, max_episode_length=7993.0),
                    dict(perturb=1), ["pert_on", "perturbation_count", "magnitude"]),
    "dt": (dict(dt=0.0025, timeout_fix=1, max_episode_length=7993.0, death_cost=-1.5),
           dict(dt=0.002), ["time", "qvel_noise", "magnitude", "obs_buf"]),
    "all": (dict(death_cost=-1.5, timeout_fix=1, max_episode_length=7993.0, initial_height=0.97, root_vel_at_com=0, dt=0.0025, perturb=0),
            dict(death_cost=0.0, timeout_fix=0, max_episode_length=8000.0, initial_height=0.93, root_vel_at_com=1, dt=0.002, perturb=1),
            ["timeout_buf", "rew_buf", "stacked_rewards", "root_states", "obs_buf", "time", "qvel_noise", "pert_on", "reset_buf"]),
}


def frozen_replay(g, backends, steps=None, recorded_noise=False):
    """Drives the backends through task_logic_frozen.npz's injected states and actions with in-kernel noise (noise = None) or,
    `recorded_noise`, the fixture's noise record (an env the fixture's own run did not reset draws zeros at its reset: the
    same words on every side); yields (t, one snapshot per backend)."""
    init = {k[5:]: v for k, v in g.items() if k.startswith("init_")}
    for be in backends:
        be.load_buffers(init)
    for t in range(int(g["steps"]) if steps is None else steps):
        for be in backends:
            if t == int(g["force_perturb_step"]):          # the population "has learned to walk": pushes start (where perturb = 1)
                ga = np.array(be.read_buffers()["gate_acc"], copy=True)
                ga[abi.K["DW_GATE_LATCH"]] = 1
                be.load_buffers({"gate_acc": ga})
            be.write_state(g["inj_root"][t], g["inj_dof"][t], g["inj_cf"][t])
            be.sim.step(g["actions"][t], g["noise"][t] if recorded_noise else None, t)
        yield (t,) + tuple(P.snapshot_buffers(be.read_buffers()) for be in backends)


def frozen_replay_pair(g, a, b, steps=None, recorded_noise=False):
    return frozen_replay(g, (a, b), steps, recorded_noise)


def assert_task_knob_bites(g, task_const, name, recorded, recorded_noise=False):
    """`recorded`: the oracle's per-step snapshots under TASK_KNOB_SETS[name].  The same replay with the set's knob back at
    its default differs in every field the knob owns, and the set reaches a time-out."""
    over, revert, owned = TASK_KNOB_SETS[name]
    base = OracleBackend(int(g["N"]), task_const, debug_freeze_physics=1, torch_gpu_div=1, **dict(over, **revert))
    differs = set()
    for t, sa in frozen_replay(g, (base,), steps=len(recorded), recorded_noise=recorded_noise):
        differs |= {k for k in owned if not np.array_equal(sa[k], recorded[t][k])}
    assert differs == set(owned), (name, sorted(set(owned) - differs))
    assert sum(int(s["timeout_buf"].sum()) for s in recorded) > 0, name


def replay(golden, backend, on_step=None):
    """Feeds the golden's inputs to `backend`, yields (t, reference_snapshot, backend_snapshot)."""
    N, steps = int(golden["N"]), int(golden["steps"])
    backend.load_buffers({k[5:]: v for k, v in golden.items() if k.startswith("init_")})
    frozen = "inj_root" in golden
    for t in range(steps):
        if frozen:
            backend.write_state(golden["inj_root"][t], golden["inj_dof"][t], golden["inj_cf"][t])
        if t == int(golden["force_perturb_step"]):
            bufs = backend.read_buffers()
            es = np.array(bufs["env_state"], copy=True)
            abi.es_view(es, "perturb_start")[...] = 1
            ga = np.array(bufs["gate_acc"], copy=True)
            ga[abi.K["DW_GATE_LATCH"]] = 1
            backend.load_buffers({"env_state": es, "gate_acc": ga})
        backend.step(golden["actions"][t], golden["noise"][t], t)
        got = P.snapshot_buffers(backend.read_buffers())
        ref = {k[5:]: v[t] for k, v in golden.items() if k.startswith("step_")}
        if t == steps - 1:
            ref.update({k[6:]: v for k, v in golden.items() if k.startswith("final_")})
        yield t, ref, got
