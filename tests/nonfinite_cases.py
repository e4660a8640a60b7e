"""Non-finite states and actions through the step kernels, shared by the CPU tests (tests/test_nonfinite.py: the oracle alone,
then the host emulation of the kernel source) and the GPU tests (tests/test_nonfinite_gpu.py): the poison table, the runner and
the checks.  Test helper; one driver serves OracleSim, EmulSim and HipSim.

What is under test is the non-finite guard of the step (csrc/dw_oct_post.h, phase post_q1; oracle/dw_task.c step_env) and the
isolation of the envs that share a wavefront with a bad env: 7 neighbours in the octet builds, 3 in the hex build, and the padding
lanes of a partial last wave, which are copies of env N - 1.  All scenes use N = 83 envs = 5 octet workgroups of 16 + 3 = 20 hex
waves of 4 + 3: the last wave is partial in every layout.  In-kernel draws (noise = None).

A run: reset_idx of every env, a scene state on top (robots on their soles, knob_cases.soles), one clean step, the poison, then
step t (the first step on the poisoned state) and two more.  The twin of a run is the same run without the poison: same build,
same seed, same actions.

Compared exactly (bit for bit) and within a bound:
  * isolation: every per-env row of every DwBuffers array, every env that was not poisoned, after each of the three steps,
    against the twin: bit for bit, no env left out.  gate_acc and the curriculum's level sums (dw_terrain_log) hold the poisoned
    env's share and are compared with the oracle's, bit for bit;
  * the poisoned env at step t against the oracle: every row bit for bit, except
      - rew_buf, stacked_rewards and last_episode_return with physics on: the reward of step t reads foot_force_pre and
        pre_joint_velocity_states, which the clean step's physics produced (the kernels' physics differs from the oracle's in
        summation order): 5e-3, test_whole_step_vs_oracle_goldens' bound on the reward;
      - on the device only (`device`), the words behind an exp / sincos / atan2, where OCML and glibc round the last bit their
        own way: rew_buf, stacked_rewards, obs_buf at replay.TRANSCENDENTAL (the golden replay's bounds), obs_history at
        (2e-6, 4e-6) as the golden replay holds it, episode_return / last_episode_return (sums of at most two rewards) at twice
        rew_buf's bound; and, for the four clean envs of the every-word scene (not reset, so their encoder words hold an in-kernel
        normal draw), DEVICE_DRAWS below;
  * the poisoned env at the two later steps, an ordinary env again, against the oracle: |dq| < 1e-4, |dqd| < 2e-2, root pose
    < 1e-4, reward < 5e-3, reset_buf equal (test_whole_step_vs_oracle_goldens);
  * finiteness of root_states, dof_state, contact_forces, obs_buf, rew_buf, stacked_rewards and the float words of env_state,
    every env, after each step.
"""
import numpy as np

import knob_cases as KC
import replay as R
from isaacgymdyros_amd import abi

N = 83
NAN, INF = float("nan"), float("inf")
STEP_REW_TOL, RUN_Q_TOL, RUN_QD_TOL, RUN_POSE_TOL = 5e-3, 1e-4, 2e-2, 1e-4      # test_whole_step_vs_oracle_goldens
OBS_HISTORY_TOL = (2e-6, 4e-6)                                                  # test_task_logic_vs_reference_goldens
# The encoder noise of an env that is not reset is a NORMAL draw, made on the device with the hardware log2 / cos (dw_task.h
# enc_normal): test_in_kernel_rng_matches_oracle_bitwise's bounds for in-kernel draws -- 2e-8 rad in qpos_noise, x 1 / dt = 1e-5
# rad/s in qvel_noise, (2e-5, 1e-5) in the observation (and so in the history rows that hold it).
DEVICE_DRAWS = dict(qpos_noise=(2e-8, 0.0), qpos_pre=(2e-8, 0.0), qvel_noise=(1e-5, 0.0), obs_buf=(2e-5, 1e-5), obs_history=(2e-5, 1e-5))
FINITE = ("root_states", "dof_state", "contact_forces", "obs_buf", "rew_buf", "stacked_rewards")
PER_ENV = [k for k, (shape, _) in abi.BUFFER_SPECS.items() if shape is not None]
ES_INT = np.zeros(abi.K["DW_ES_WORDS"], bool)
for _name, (_off, _shape, _kind) in abi.ES_FIELDS.items():
    if _kind == "i":
        ES_INT[_off:_off + int(np.prod(_shape, dtype=int))] = True

# ---------------------------------------------------------------- the poison table: (buffer, index within the env's row, value)
POISONS = {
    "quat_nan": ("root_states", 3, NAN),
    "x_nan": ("root_states", 0, NAN),
    "vel_inf": ("root_states", 8, INF),
    "q32_inf": ("dof_state", 2 * 32, INF),
    "qd5_nan": ("dof_state", 2 * 5 + 1, NAN),
    "qd3_big": ("dof_state", 2 * 3 + 1, 3e38),          # finite: overflows inside the step, the guard sees what the physics left
}
PLACEMENTS = {
    "env_0": (0,),
    "octet_wave_edge": (7, 8),
    "workgroup_edge": (15, 16),
    "hex_wave_edge": (3, 4),
    "last_env": (N - 1,),                               # the padding lanes of the last wave are its copies
    "two_in_a_wave": (24, 25),
    "whole_wave": tuple(range(32, 40)),
}
# Each poison at the placements that distinguish it.  The root words are scanned and rewritten by the env's own first lane; the joint
# words by item lanes, item (env, joint) = lane + 64 k, whose env is a division of the item index: the joint poisons take every edge
# between envs, waves and workgroups, the root poisons one of each kind between them.  Every poison runs at env N - 1.
PLACEMENT_SCENES = (
    [("quat_nan", p) for p in ("env_0", "octet_wave_edge", "last_env", "whole_wave")]
    + [("x_nan", p) for p in ("hex_wave_edge", "workgroup_edge", "last_env")]
    + [("vel_inf", p) for p in ("env_0", "two_in_a_wave", "last_env")]
    + [("q32_inf", p) for p in PLACEMENTS]
    + [("qd5_nan", p) for p in ("env_0", "hex_wave_edge", "workgroup_edge", "last_env", "whole_wave")]
    + [("qd3_big", p) for p in ("octet_wave_edge", "two_in_a_wave", "last_env")])
ACTION_SCENES = [(col, v) for col in (4, 12) for v in (NAN, INF, -INF)]
ACTION_ENV = 24
TERRAIN_POISONS = {"x_nan": [("root_states", 0, NAN)], "y_inf": [("root_states", 1, INF)],
                   "x_nan_y_inf": [("root_states", 0, NAN), ("root_states", 1, INF)]}
TERRAIN_SCENES = [(p, e) for p in TERRAIN_POISONS for e in (11, N - 1)]
SIMULATE_POISONS = {"quat_nan": ("root_states", 3, NAN), "q7_inf": ("dof_state", 2 * 7, INF)}
SIMULATE_ENV, SIMULATE_SUBSTEPS = 24, 3


def scene_id(s):
    return "-".join(str(x) for x in s)


def every_word_poison():
    """Env w + 1 is poisoned in state word w (0..12 root_states, 13..78 dof_state), values cycling NaN, +Inf, -Inf."""
    vals = (NAN, INF, -INF)
    return [(w + 1, "root_states" if w < 13 else "dof_state", w if w < 13 else w - 13, vals[w % 3]) for w in range(79)]


# ---------------------------------------------------------------- terrains
_terrains = {}


def terrain(kind):
    if kind is None:
        return None
    if kind not in _terrains:
        if kind == "slope":
            _terrains[kind] = KC.SlopeField()
        else:
            # a generated curriculum map (what with_terrain(cfg, mesh_type="heightfield", curriculum=True, ...) builds): 3 levels x 4 types
            from isaacgymdyros_amd.terrain import Terrain, TerrainCfg
            _terrains[kind] = Terrain(TerrainCfg(mesh_type="heightfield", curriculum=True, num_rows=3, num_cols=4, border_size=5.0), N, seed=4)
    return _terrains[kind]


# ---------------------------------------------------------------- the runner
def actions(t):
    return np.random.default_rng(100 + t).uniform(-1.0, 1.0, size=(N, 13)).astype(np.float32)


def _start(sim, kind, field):
    """reset_idx of every env, then the scene: robots on their soles (plane, slope) or as the reset spawned them (curriculum map)."""
    b = sim.buf
    if kind == "slope":
        b["env_origins"][:] = np.array([0.0, 0.0, field.height(1.0)], np.float32)          # a reset spawns within 1 m of it, above the slope
    elif kind == "curriculum":
        c = field.cfg
        ty = np.minimum(np.arange(N) * c.num_cols // N, c.num_cols - 1)
        lv = np.arange(N) % 2
        b["terrain_types"][:], b["terrain_levels"][:] = ty, lv
        b["env_origins"][:] = np.asarray(field.env_origins, np.float32).reshape(c.num_rows, c.num_cols, 3)[lv, ty]
    # (a reset forms contact_reward_mean = contact_reward_sum / epi_len: 0 / 0 on a record that has never stepped, as in the reference)
    abi.es_view(b["env_state"], "epi_len")[...] = 1.0
    sim.reset_idx(np.arange(N, dtype=np.int32), None, 0)
    if kind != "curriculum":
        st = KC.soles(N, np.random.default_rng(7), speed=(0.0, 0.3), field=field)
        for k, v in st.items():
            b[k][...] = np.asarray(v, np.float32).reshape(b[k].shape)
        b["contact_forces"][...] = 0


def _level_means(sim, levels):
    """The curriculum's logging columns as the reference forms them (tasks/dyros_dynamic_walk.py:417-421): the mean level of the envs
    of each terrain type, from the levels BEFORE the step's resets move any (the oracle library has no dw_terrain_log: this is its side)."""
    types = int(sim.cfg.terrain_num_types)
    ty = np.clip(sim.buf["terrain_types"], 0, types - 1)
    out = np.zeros(types, np.float32)
    for t in range(types):
        cnt, tot = np.float32(max(int((ty == t).sum()), 1)), np.float32(levels[ty == t].sum())
        out[t] = tot * (np.float32(1.0) / cnt) if sim.cfg.torch_gpu_div else tot / cnt
    return out


def _snap(sim, levels_before):
    s = {k: np.array(v, copy=True) for k, v in sim.buf.items()}
    if levels_before is not None:
        s["level_means"] = _level_means(sim, levels_before)
        if "terrain_log" in sim.api:
            s["terrain_log"] = sim.terrain_log()
    return s


def _put(sim, env, buffer, index, value):
    sim.buf[buffer].reshape(N, -1)[env, index] = np.float32(value)


def run_step_scene(make, kind=None, freeze=0, poison=(), action_poison=()):
    """poison: (env, buffer, index, value) written after the clean step; action_poison: (env, column, value) put into the
    actions of step t.  Returns the snapshots after step t and the two later steps."""
    field = terrain(kind)
    cfg = dict(debug_freeze_physics=freeze)
    if kind == "slope":
        cfg["terrain_curriculum"] = 0
    sim = make(N, terrain=field, **cfg)
    try:
        _start(sim, kind, field)
        sim.step(actions(0), None, 1)
        for env, buffer, index, value in poison:
            _put(sim, env, buffer, index, value)
        out = []
        for t in (1, 2, 3):
            a = actions(t)
            if t == 1:
                for env, col, value in action_poison:
                    a[env, col] = value
            levels = sim.buf["terrain_levels"].copy() if kind == "curriculum" else None
            sim.step(a, None, t + 1)
            out.append(_snap(sim, levels))
        return out
    finally:
        if hasattr(sim, "close"):
            sim.close()


def run_simulate_scene(make, kind, poison=()):
    """dw_simulate, no guard: the soles scene, SIMULATE_SUBSTEPS substeps at zero joint torque; the state and forces after the last."""
    field = terrain(kind)
    cfg = dict(self_collision=0)
    if kind == "slope":
        cfg["terrain_curriculum"] = 0
    sim = make(N, terrain=field, **cfg)
    try:
        st = KC.soles(N, np.random.default_rng(5), field=field)
        for k, v in st.items():
            sim.buf[k][...] = np.asarray(v, np.float32).reshape(sim.buf[k].shape)
        for env, buffer, index, value in poison:
            _put(sim, env, buffer, index, value)
        tau = np.zeros((N, 33), np.float32)
        for _ in range(SIMULATE_SUBSTEPS):
            sim.simulate(tau)
        return {k: sim.buf[k].copy() for k in ("root_states", "dof_state", "contact_forces")}
    finally:
        if hasattr(sim, "close"):
            sim.close()


_runs = {}


def cached(label, fn, make, *key, **kw):
    """One run per (backend label, scene): the twins and the oracle's runs are shared by the tests that need them, and left unchanged."""
    k = (label, fn.__name__) + key + tuple(sorted((a, repr(b)) for a, b in kw.items()))
    if k not in _runs:
        _runs[k] = fn(make, *key, **kw)
    return _runs[k]


# ---------------------------------------------------------------- checks
def _rows(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(N, -1)


def differing_rows(a, b, envs, buffers=PER_ENV):
    """{buffer: envs of `envs` whose row differs in any bit}."""
    envs = np.asarray(envs, int)
    out = {}
    for k in buffers:
        d = (_rows(a[k])[envs] != _rows(b[k])[envs]).any(axis=1)
        if d.any():
            out[k] = envs[d].tolist()
    return out


def assert_finite(snap, where):
    for k in FINITE:
        bad = np.nonzero(~np.isfinite(snap[k].reshape(N, -1)).all(axis=1))[0]
        assert bad.size == 0, (where, k, bad.tolist())
    es = snap["env_state"][:, ~ES_INT]
    bad = np.nonzero(~np.isfinite(es).all(axis=1))[0]
    assert bad.size == 0, (where, "env_state", bad.tolist())


def nan_resets(snap):
    return abi.es_view(snap["env_state"], "nan_resets")


def _close(a, b, tol):
    ab, rl = tol
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= ab + rl * np.abs(a)))


def assert_rows_equal_oracle(got, ref, envs, where, physics, device, draws=False):
    """The rows of `envs` after step t against the oracle's: bit for bit but for the words the module docstring lists.  draws: the
    envs were not reset in step t, so their encoder words hold an in-kernel normal draw."""
    envs = np.asarray(envs, int)
    if len(envs) == 0:
        return
    loose = {}
    if physics:
        loose.update(rew_buf=(STEP_REW_TOL, 0.0), stacked_rewards=(STEP_REW_TOL, 0.0), last_episode_return=(STEP_REW_TOL, 0.0))
    elif device:
        rb = R.TRANSCENDENTAL["rew_buf"]
        loose.update(rew_buf=rb, stacked_rewards=R.TRANSCENDENTAL["stacked_rewards"], last_episode_return=(2 * rb[0], 2 * rb[1]),
                     episode_return=(2 * rb[0], 2 * rb[1]))
    if device:
        loose.update(obs_buf=R.TRANSCENDENTAL["obs_buf"], obs_history=OBS_HISTORY_TOL)
    if device and draws:
        loose.update(DEVICE_DRAWS)
    es_loose = np.zeros(abi.K["DW_ES_WORDS"], bool)
    for k in loose:
        if k in abi.ES_FIELDS:
            off, shape, _ = abi.ES_FIELDS[k]
            es_loose[off:off + int(np.prod(shape, dtype=int))] = True
    for k in PER_ENV:
        a, b = ref[k].reshape(N, -1)[envs], got[k].reshape(N, -1)[envs]
        if k == "env_state":
            for name in loose:
                if name in abi.ES_FIELDS:
                    assert _close(abi.es_view(ref[k], name)[envs], abi.es_view(got[k], name)[envs], loose[name]), (where, name)
            a, b = a[:, ~es_loose], b[:, ~es_loose]
        elif k in loose:
            assert _close(a, b, loose[k]), (where, k, float(np.abs(a.astype(np.float64) - b).max()))
            continue
        same = np.ascontiguousarray(a).view(np.uint8).reshape(len(envs), -1) == np.ascontiguousarray(b).view(np.uint8).reshape(len(envs), -1)
        if not same.all():          # (which env, which 4-byte word of its row, both values)
            e, w = np.argwhere(~same.reshape(len(envs), -1, a.dtype.itemsize).all(axis=2))[0]
            cols = np.nonzero(~es_loose)[0] if k == "env_state" else np.arange(a.shape[1])
            raise AssertionError((where, k, "envs", envs[~same.all(axis=1)].tolist(), "first: env %d word %d oracle %r got %r" % (envs[e], cols[w], a[e, w], b[e, w])))


def check_guarded_scene(label, make, oracle_make, kind, poison, device=False, freeze=0, expect_resets=1):
    """A step scene with state poison on `label`'s backend: isolation against the twin, outcome / reset rows / later steps of the
    poisoned envs and the cross-env sums against the oracle, finiteness."""
    bad = sorted({p[0] for p in poison})
    clean = np.setdiff1d(np.arange(N), bad)
    got = run_step_scene(make, kind, freeze, poison=tuple(poison))
    twin = cached(label, run_step_scene, make, kind, freeze)
    ref = cached("oracle", run_step_scene, oracle_make, kind, freeze, poison=tuple(poison))
    for t, (g, w, r) in enumerate(zip(got, twin, ref)):
        where = (label, kind, "step t + %d" % t)
        assert_finite(g, where)
        # isolation: every row of every env that was not poisoned, bit for bit against the twin
        diff = differing_rows(g, w, clean)
        assert not diff, (where, "rows that differ from the twin's", diff)
        # the cross-env sums hold the poisoned env's share: against the oracle
        assert np.array_equal(g["gate_acc"], r["gate_acc"]), (where, "gate_acc")
        if "terrain_log" in g:
            assert g["terrain_log"].shape == (N, 15 + len(r["level_means"])), where
            assert np.array_equal(g["terrain_log"][:, 15:], np.tile(r["level_means"], (N, 1))), (where, "dw_terrain_log", g["terrain_log"][0, 15:], r["level_means"])
            assert np.array_equal(g["terrain_log"][:, :15], g["stacked_rewards"]), where
        # outcome
        for k in ("reset_buf", "progress_buf", "timeout_buf", "randomize_buf", "terrain_levels"):
            assert np.array_equal(g[k][bad], r[k][bad]), (where, k, g[k][bad], r[k][bad])
        for name in ("nan_resets", "episodes_finished"):
            assert np.array_equal(abi.es_view(g["env_state"], name)[bad], abi.es_view(r["env_state"], name)[bad]), (where, name)
        nr = nan_resets(g)
        assert (nr[bad] == expect_resets).all() and (nr[clean] == 0).all(), (where, "nan_resets", nr.tolist())
        if t == 0:
            assert (g["reset_buf"][bad] == 1).all() and (g["progress_buf"][bad] == 0).all(), (where, "the poisoned envs are reset in step t")
            # reset rows (and every other row of the poisoned envs) against the oracle
            assert_rows_equal_oracle(g, r, bad, where, physics=not freeze, device=device)
        elif not freeze:
            # an ordinary env again: the bounds of test_whole_step_vs_oracle_goldens
            dq = np.abs(g["dof_state"][bad, :, 0] - r["dof_state"][bad, :, 0]).max()
            dqd = np.abs(g["dof_state"][bad, :, 1] - r["dof_state"][bad, :, 1]).max()
            pose = np.abs(g["root_states"][bad, :7] - r["root_states"][bad, :7]).max()
            rew = np.abs(g["rew_buf"][bad] - r["rew_buf"][bad]).max()
            print("%-10s %-10s t + %d poisoned envs vs oracle: dq %.2e dqd %.2e pose %.2e rew %.2e" % (label, kind, t, dq, dqd, pose, rew))
            assert dq < RUN_Q_TOL and dqd < RUN_QD_TOL and pose < RUN_POSE_TOL and rew < STEP_REW_TOL, (where, dq, dqd, pose, rew)
    return got, ref


def check_every_word(label, make, oracle_make, device=False):
    """Physics frozen, env w + 1 poisoned in state word w: after step t every buffer equals the oracle's (bit for bit; on the device
    the words behind a transcendental at the golden replay's bounds), one counted reset on each of envs 1 .. 79."""
    poison = every_word_poison()
    got = run_step_scene(make, None, 1, poison=tuple(poison))[0]
    ref = cached("oracle", run_step_scene, oracle_make, None, 1, poison=tuple(poison))[0]
    assert_finite(got, (label, "every word"))
    bad = np.arange(1, 80)
    assert_rows_equal_oracle(got, ref, bad, (label, "every word"), physics=False, device=device)
    assert_rows_equal_oracle(got, ref, np.setdiff1d(np.arange(N), bad), (label, "every word, clean envs"), physics=False, device=device, draws=True)
    assert np.array_equal(got["gate_acc"], ref["gate_acc"]), (label, "gate_acc")
    nr = nan_resets(got)
    assert (nr[1:80] == 1).all() and nr[0] == 0 and (nr[80:] == 0).all(), nr.tolist()
    assert (got["reset_buf"][1:80] == 1).all()
    assert np.array_equal(got["reset_buf"], ref["reset_buf"])


def check_action_scene(label, make, oracle_make, col, value):
    """A non-finite action word of env ACTION_ENV in step t: swallowed by the action clamp (no reset, everything finite), the env's
    clamped actions and counters equal the oracle's, the neighbours the twin's."""
    ap = ((ACTION_ENV, col, value),)
    got = run_step_scene(make, action_poison=ap)
    twin = cached(label, run_step_scene, make, None, 0)
    ref = cached("oracle", run_step_scene, oracle_make, action_poison=ap)
    clean = np.setdiff1d(np.arange(N), [ACTION_ENV])
    for t, (g, w, r) in enumerate(zip(got, twin, ref)):
        where = (label, "action", col, value, "step t + %d" % t)
        assert_finite(g, where)
        assert_finite(r, where + ("oracle",))
        diff = differing_rows(g, w, clean)
        assert not diff, (where, "rows that differ from the twin's", diff)
        for name in ("actions", "actions_pre", "nan_resets", "episodes_finished"):
            a, b = abi.es_view(g["env_state"], name)[ACTION_ENV], abi.es_view(r["env_state"], name)[ACTION_ENV]
            assert np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32)), (where, name, a, b)
        for k in ("reset_buf", "progress_buf", "timeout_buf", "randomize_buf"):
            assert g[k][ACTION_ENV] == r[k][ACTION_ENV], (where, k)
        assert not nan_resets(g).any() and not nan_resets(r).any(), where
        assert r["reset_buf"][ACTION_ENV] == 0, where


def check_simulate_scene(label, make, kind, poison_name):
    """dw_simulate has no guard: the neighbours of a non-finite env are bit-identical to the twin's; nothing is asserted about the env."""
    buffer, index, value = SIMULATE_POISONS[poison_name]
    got = run_simulate_scene(make, kind, poison=((SIMULATE_ENV, buffer, index, value),))
    twin = cached(label, run_simulate_scene, make, kind)
    clean = np.setdiff1d(np.arange(N), [SIMULATE_ENV])
    diff = differing_rows(got, twin, clean, buffers=("root_states", "dof_state", "contact_forces"))
    assert not diff, (label, kind, poison_name, diff)
    assert all(np.isfinite(got[k][clean]).all() for k in got)


# ---------------------------------------------------------------- the fused TocabiAMPLower step (no guard, as the reference)
AMP_N, AMP_ENV, AMP_STEPS_BEFORE, AMP_STEPS_AFTER = 37, 5, 2, 3
AMP_GYM = ("root_states", "dof_state", "contact_forces", "dof_damping", "dof_armature")


def run_amp_emul(poison):
    """AmpEmul over the octet emulation (the two-waves build, as the one-launch step on the device): AMP_STEPS_BEFORE steps, env
    AMP_ENV's joint angles set to NaN, AMP_STEPS_AFTER more; every table of abi.AMP_BUFFER_NAMES and the Gym tensors."""
    from amp_emul import AmpEmul
    from emul_backend import EmulSim
    sim = EmulSim(AMP_N, self_collision=0, debug_wave_build=2)
    env = AmpEmul(sim, AMP_N)
    rng = np.random.default_rng(4)
    for t in range(AMP_STEPS_BEFORE + AMP_STEPS_AFTER):
        env.reset_done()
        if poison and t == AMP_STEPS_BEFORE:
            sim.buf["dof_state"][AMP_ENV, :, 0] = NAN
        env.step((rng.random((AMP_N, 12), dtype=np.float32) * 2 - 1) * 0.7)
    out = {n: env.a[n].copy() for n in abi.AMP_BUFFER_NAMES}
    out.update({"gym_" + k: sim.buf[k].copy() for k in AMP_GYM})
    return out


def check_amp_isolation(got, twin):
    """Every table, the rows of the AMP_N - 1 envs that were not poisoned (tables without an env dimension: the whole table): bit for bit."""
    assert set(got) == set(twin) and all(("gym_" + k) in got for k in AMP_GYM)
    clean = np.setdiff1d(np.arange(AMP_N), [AMP_ENV])
    for n in got:
        a, b = np.ascontiguousarray(got[n]), np.ascontiguousarray(twin[n])
        assert a.shape == b.shape and a.dtype == b.dtype, n
        if a.ndim and a.shape[0] == AMP_N:
            a, b = a[clean], b[clean]
        same = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1) == np.ascontiguousarray(b).view(np.uint8).reshape(b.shape[0], -1)
        assert same.all(), (n, np.nonzero(~same.all(axis=1))[0].tolist())
    # (the scene is live: the poisoned env's own rows differ from the twin's)
    assert not np.array_equal(got["obs_buf"][AMP_ENV], twin["obs_buf"][AMP_ENV])
