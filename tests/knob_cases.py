"""Physics cases away from the default DwConfig, shared by the CPU emulation tests (tests/test_kernel_emulation.py) and
the GPU tests (tests/test_hip_gpu.py): a case = config overrides + a seeded scene + what is compared against the oracle
after ONE substep (state and net contact forces) and after a short run (state).  Test helper.

Every case proves first that its knob bites (`assert_bites`): the oracle with the override and the oracle with the
default value, on the same scene, differ by >= 20 x the tolerance in at least one compared quantity -- otherwise a kernel
that ignored the field would pass.

Tolerances (DESIGN.md sections 3 / 4, none derived from a kernel):
  * one substep: the state 1e-5 against the fp32 oracle, positions (root pose, q) and velocities (root velocity, qd) alike.
    Where the velocities of a case do not meet 1e-5 (every case with contact: the fp32 oracle's own velocities differ from
    the fp64 oracle's by 5e-5 .. 2.5e-4 there), they are compared with the fp64 oracle instead and held to 4 x the
    fp32-oracle-to-fp64-oracle difference on the same scene, computed in the test: one figure per case, the largest
    difference over all 39 velocity entries of the state (root velocity and qd: they are coupled through the same contact
    impulses), as the project bound is one figure for the state.  Net contact forces 1e-3 relative on bodies the oracle
    loads above 50 N, and for SOLES on the friction cone (the two foot bodies, |Ft| > 0.95 mu Fn, mu > 0) the percentile
    bounds of test_sliding_sole_contacts_with_friction_dr_vs_oracle: 5e-4 median, 3e-3 99th, 1e-2 worst;
  * short run (RUN_SUBSTEPS = 20 substeps = 10 policy steps): |dq| <= 1e-4 rad, |dqd| <= 2e-2 rad/s, root pose <= 1e-4,
    root velocity <= 2e-2 (test_whole_step_vs_oracle_goldens' bounds for the same horizon).
"""
import numpy as np

from isaacgymdyros_amd.task_constants import INITIAL_DOF_POS
from oracle.oracle import OracleSim

STATE_TOL, FP64_FACTOR, FORCE_REL, LOADED_N = 1e-5, 4.0, 1e-3, 50.0
CONE_P50, CONE_P99, CONE_MAX = 5e-4, 3e-3, 1e-2
RUN_SUBSTEPS, RUN_POS_TOL, RUN_VEL_TOL = 20, 1e-4, 2e-2
BITE = 20.0


class SlopeField:
    """A uniform 3 % slope along x with the attributes OracleSim(terrain=...) reads (the height-field instantiation of the
    kernels; 0.1 m grid, 5 mm height quantum)."""
    SLOPE, BORDER = 0.03, 4.0

    def __init__(self):
        from isaacgymdyros_amd.terrain import TerrainCfg
        rows = np.arange(80).reshape(-1, 1) * np.ones((1, 80))
        self.heightsamples = np.ascontiguousarray(np.rint(rows * 0.1 * self.SLOPE / 0.005), dtype=np.int16)
        self.tot_rows, self.tot_cols = self.heightsamples.shape
        self.env_length = 8.0
        self.env_origins = np.zeros((1, 1, 3))
        self.cfg = TerrainCfg(mesh_type="heightfield", horizontal_scale=0.1, vertical_scale=0.005, border_size=self.BORDER,
                              curriculum=False, num_rows=1, num_cols=1)

    def height(self, x):
        return self.SLOPE * (x + self.BORDER)


# ---------------------------------------------------------------- scenes: (N, rng) -> {buffer: array}
def _base(N):
    root = np.zeros((N, 13), np.float32)
    root[:, 6] = 1.0
    dof = np.zeros((N, 33, 2), np.float32)
    dof[:, :, 0] = np.asarray(INITIAL_DOF_POS, np.float32)
    return root, dof


def soles(N, rng, depth=(0.0001, 0.004), speed=(0.0, 1.0), vz=0.0, spin=0.3, mu_scale=None, field=None):
    """Robots on their soles (the sole plane of the initial pose lies 0.9286 m under the base origin): penetrations drawn
    from `depth` (negative = hovering), a horizontal base velocity of `speed` in a random direction (above ~0.3 m/s the
    soles slide), a vertical one of `vz`, joints within 0.02 rad of the initial pose, joint rates ~0.2 rad/s."""
    root, dof = _base(N)
    root[:, 0:2] = rng.uniform(-1, 1, size=(N, 2))
    root[:, 2] = 0.9286 - rng.uniform(depth[0], depth[1], N)
    if field is not None:
        root[:, 2] += field.height(root[:, 0])
    ang, spd = rng.uniform(0, 2 * np.pi, N), rng.uniform(speed[0], speed[1], N)
    root[:, 7], root[:, 8], root[:, 9] = spd * np.cos(ang), spd * np.sin(ang), vz
    root[:, 10:13] = rng.normal(size=(N, 3)) * spin
    dof[:, :, 0] += rng.normal(size=(N, 33)) * 0.02
    dof[:, :, 1] = rng.normal(size=(N, 33)) * 0.2
    out = {"root_states": root, "dof_state": dof}
    if mu_scale is not None:
        out["friction_scale"] = rng.uniform(mu_scale[0], mu_scale[1], N).astype(np.float32)
    return out


def flight(N, rng, spin=0.5):
    """Three metres up, random attitude, base rates ~`spin`, joints within 0.5 rad of the initial pose."""
    root, dof = _base(N)
    root[:, 0:3] = rng.normal(size=(N, 3)) * 0.5 + np.array([0, 0, 3.0])
    q = rng.normal(size=(N, 4))
    root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    root[:, 7:10] = rng.normal(size=(N, 3)) * 0.5
    root[:, 10:13] = rng.normal(size=(N, 3)) * spin
    dof[:, :, 0] += rng.uniform(-0.5, 0.5, size=(N, 33))
    dof[:, :, 1] = rng.uniform(-1, 1, size=(N, 33))
    return {"root_states": root, "dof_state": dof}


def pelvis_in_ground(N, rng):
    """The scene of test_oracle_physics.py::test_non_foot_contact_is_reported over a range of depths: all joints at zero,
    base origin 5 .. 30 mm under the plane (the pelvis' and the leg links' primitives are in the ground: the penalty
    model's contacts), drifting at up to 0.3 m/s."""
    root, dof = _base(N)
    dof[:, :, 0] = 0.0
    root[:, 2] = -rng.uniform(0.005, 0.03, N)
    root[:, 7:10] = rng.uniform(-0.3, 0.3, size=(N, 3))
    return {"root_states": root, "dof_state": dof}


def crossed_legs(N, rng):
    """Skew shank capsules interpenetrating (tests/test_kernel_emulation.py::_crossed, asymmetric form), in flight, the
    legs closing on each other at up to 1 rad/s in hip roll so that the penalty damping term works."""
    root, dof = _base(N)
    root[:, 2] = 3.0
    roll = np.linspace(0.05, 0.25, N).astype(np.float32)
    dof[:, 1, 0], dof[:, 7, 0] = -roll, roll
    dof[:, 6, 0] = 0.15
    dof[:, 8, 0] += 0.25
    rate = rng.uniform(0.2, 1.0, N)
    dof[:, 1, 1], dof[:, 7, 1] = -rate, rate
    return {"root_states": root, "dof_state": dof}


# ---------------------------------------------------------------- the table
def _case(over, scene, seed, **fixed):
    """over: the knobs of the case; fixed: configuration both the override run and the default run of the bite check get."""
    return dict(over=over, scene=scene, seed=seed, fixed=dict({"self_collision": 0}, **fixed))


_FIELD = SlopeField()
ALL_OFF_DEFAULT = dict(solver_iterations=9, erp=0.5, max_depenetration_velocity=0.4, contact_offset=0.006, contact_cfm=0.3,
                       friction=0.6, gravity=(1.2, -0.8, -9.2), dt=0.0025, max_angular_velocity=50.0, root_vel_at_com=0,
                       penalty_stiffness=6e4, penalty_damping=4e2)

CASES = {
    # the Gauss-Seidel trip count: loaded soles, some sliding
    "iters_1": _case(dict(solver_iterations=1), soles, 5),
    "iters_12": _case(dict(solver_iterations=12), soles, 5),
    "iters_64": _case(dict(solver_iterations=64), soles, 5),
    # fminf(erp depth / dt, max_depen): 0.1 .. 6 mm deep; 0.8 x depth / 2 ms = 0.04 .. 2.4 m/s against a cap of 0.5 m/s
    "erp_and_depenetration_cap": _case(dict(erp=0.8, max_depenetration_velocity=0.5),
                                       lambda N, rng: soles(N, rng, depth=(0.0001, 0.006), speed=(0.0, 0.3)), 6),
    # soles hovering 2.5 .. 6 mm over the plane (outside the default 2 mm margin), falling at 4 m/s: -phi/dt = -1.25 .. -3 m/s
    "contact_offset": _case(dict(contact_offset=0.02),
                            lambda N, rng: soles(N, rng, depth=(-0.006, -0.0025), speed=(0.0, 0.2), vz=-4.0), 7),
    "contact_cfm": _case(dict(contact_cfm=2.0), soles, 8),
    "friction_0": _case(dict(friction=0.0), lambda N, rng: soles(N, rng, speed=(0.3, 1.0), mu_scale=(0.7, 1.3)), 9),
    "friction_0.3": _case(dict(friction=0.3), lambda N, rng: soles(N, rng, speed=(0.3, 1.0), mu_scale=(0.7, 1.3)), 9),
    "gravity_xy_flight": _case(dict(gravity=(3.0, -4.0, -7.0)), flight, 10),
    "gravity_xy_stance": _case(dict(gravity=(3.0, -4.0, -7.0)), soles, 11),
    "dt_0.001": _case(dict(dt=0.001), soles, 12),
    "dt_0.004": _case(dict(dt=0.004), soles, 12),
    # base spinning at ~5 rad/s per axis: the clamp rescales nearly every env
    "max_angular_velocity": _case(dict(max_angular_velocity=2.0), lambda N, rng: flight(N, rng, spin=5.0), 13),
    "root_vel_at_origin": _case(dict(root_vel_at_com=0), lambda N, rng: flight(N, rng, spin=3.0), 14),
    "penalty_ground": _case(dict(penalty_stiffness=3e4, penalty_damping=3e2), pelvis_in_ground, 15),
    "penalty_self_collision": _case(dict(penalty_stiffness=3e4, penalty_damping=3e2), crossed_legs, 16, self_collision=1),
    # everything off default at once, on the height field (a different instantiation of the kernels)
    "all_on_terrain": _case(ALL_OFF_DEFAULT, lambda N, rng: soles(N, rng, depth=(-0.004, 0.004), speed=(0.0, 1.0), vz=-1.0,
                                                                  mu_scale=(0.7, 1.3), field=_FIELD),
                            17, terrain=_FIELD, terrain_curriculum=0),
}
N_ENVS = 64
# cases whose scene touches nothing: no force comparison to demand, and the velocities meet the project bound as it stands
NO_CONTACT = ("gravity_xy_flight", "max_angular_velocity", "root_vel_at_origin")
# cases that move a pair of knobs: each of the two is shown to bite alone as well
EACH_KNOB_BITES = ("erp_and_depenetration_cap", "penalty_ground", "penalty_self_collision")


def case_config(name, with_override=True, revert=None):
    """The case's configuration; with_override = False: every knob at its default; revert: that one knob at its default."""
    c = CASES[name]
    over = {k: v for k, v in c["over"].items() if k != revert} if with_override else {}
    return dict(c["fixed"], **over)


def load_scene(sim, name):
    """Writes the case's scene into sim.buf (numpy buffers of an OracleSim / EmulSim / HipSim)."""
    c = CASES[name]
    scene = c["scene"](sim.N, np.random.default_rng(c["seed"]))
    for k, v in scene.items():
        sim.buf[k][...] = np.asarray(v, np.float32).reshape(sim.buf[k].shape)
    sim.buf["contact_forces"][...] = 0


def run_case(sim, name):
    """ONE substep and then the rest of the short run, zero joint torque; returns (state and forces after one substep, state
    after RUN_SUBSTEPS)."""
    load_scene(sim, name)
    tau = np.zeros((sim.N, 33), np.float32)
    sim.simulate(tau)
    one = {k: sim.buf[k].copy() for k in ("root_states", "dof_state", "contact_forces")}
    for _ in range(RUN_SUBSTEPS - 1):
        sim.simulate(tau)
    return one, {k: sim.buf[k].copy() for k in ("root_states", "dof_state")}


_oracle_runs = {}


def oracle_run(name, task_const, with_override=True, double=False, revert=None):
    """The oracle's result of a case (cached: the emulation tests ask once per wave build)."""
    key = (name, with_override, double, revert)
    if key not in _oracle_runs:
        cfg = dict(case_config(name, with_override, revert))
        terrain = cfg.pop("terrain", None)
        sim = OracleSim(N_ENVS, task_const=task_const, double=double, terrain=terrain, **cfg)
        one, run = run_case(sim, name)
        _oracle_runs[key] = (one, run, float(sim.cfg.friction) * sim.buf["friction_scale"].reshape(sim.N).copy())
    return _oracle_runs[key]


# ---------------------------------------------------------------- comparisons
def _state_diffs(a, b):
    return {"root pose": np.abs(a["root_states"][:, :7] - b["root_states"][:, :7]).max(),
            "q": np.abs(a["dof_state"][:, :, 0] - b["dof_state"][:, :, 0]).max(),
            "root velocity": np.abs(a["root_states"][:, 7:] - b["root_states"][:, 7:]).max(),
            "qd": np.abs(a["dof_state"][:, :, 1] - b["dof_state"][:, :, 1]).max()}


def _velocity_diff(a, b):
    """The largest difference over the velocity entries of the state (root velocity and qd)."""
    d = _state_diffs(a, b)
    return float(max(d["root velocity"], d["qd"]))


def velocity_bound(name, task_const):
    """(fp32-oracle-to-fp64-oracle velocity difference of the case after one substep, the bound on a kernel's distance from
    the fp64 oracle that follows from it)."""
    d = _velocity_diff(oracle_run(name, task_const)[0], oracle_run(name, task_const, double=True)[0])
    return d, FP64_FACTOR * d


def _feet():
    from isaacgymdyros_amd.model import load_model
    m = load_model()
    return (m.left_foot_idx, m.right_foot_idx)


def _force_rel(ref, got, mu):
    """Per (env, body) the oracle loads above LOADED_N: relative difference, whether the pair is a sole on the friction
    cone, the env index."""
    mag = np.linalg.norm(ref, axis=2)
    e, b = np.nonzero(mag > LOADED_N)
    rel = np.abs(got[e, b] - ref[e, b]).max(axis=1) / mag[e, b]
    ft, fn = np.linalg.norm(ref[e, b, :2], axis=1), ref[e, b, 2]
    cone = np.isin(b, _feet()) & (mu[e] > 0) & (fn > 0) & (ft > 0.95 * mu[e] * fn)
    return rel, cone, e


def _bite_ratios(a, b, vel_tol):
    """Differences between two oracle results (one substep, short run) over the tolerance each quantity is held to."""
    (one_a, run_a, _), (one_b, run_b, _) = a, b
    ratios = {k: v / (STATE_TOL if k in ("root pose", "q") else vel_tol) for k, v in _state_diffs(one_a, one_b).items()}
    fa, fb = one_a["contact_forces"], one_b["contact_forces"]
    big = np.maximum(np.linalg.norm(fa, axis=2), np.linalg.norm(fb, axis=2))
    sel = big > LOADED_N
    ratios["forces"] = (np.abs(fa - fb).max(axis=2)[sel] / big[sel]).max() / FORCE_REL if sel.any() else 0.0
    ratios.update({"run " + k: v / (RUN_POS_TOL if k in ("root pose", "q") else RUN_VEL_TOL)
                   for k, v in _state_diffs(run_a, run_b).items()})
    return ratios


def assert_bites(name, task_const):
    """The knob-bites condition: the oracle with and without the override differ by >= BITE x the tolerance somewhere (the
    one-substep velocities at the looser of the case's two bounds, 1e-5 and 4 x the fp32 / fp64 oracle difference).  Where
    a case moves a pair of knobs (erp with the depenetration cap, penalty stiffness with damping), each knob alone,
    reverted to its default with the other kept, bites too."""
    vel_tol = max(STATE_TOL, velocity_bound(name, task_const)[1])
    full = oracle_run(name, task_const)
    ratios = _bite_ratios(full, oracle_run(name, task_const, with_override=False), vel_tol)
    print("%-26s bite (difference / tolerance; velocity tolerance %.2e): %s" % (name, vel_tol, "  ".join("%s %.3g" % kv for kv in ratios.items())))
    assert max(ratios.values()) >= BITE, (name, ratios)
    if name in EACH_KNOB_BITES:
        for field in CASES[name]["over"]:
            r = _bite_ratios(full, oracle_run(name, task_const, revert=field), vel_tol)
            print("%-26s   %s alone: largest %.3g (%s)" % (name, field, max(r.values()), max(r, key=r.get)))
            assert max(r.values()) >= BITE, (name, field, r)
    return ratios


def assert_both_cap_branches(name="erp_and_depenetration_cap"):
    """fminf(erp depth / dt, max_depen): the scene's penetrations put a good share of the envs on either side of the cap."""
    c = CASES[name]
    root = c["scene"](N_ENVS, np.random.default_rng(c["seed"]))["root_states"]
    cap = c["over"]["max_depenetration_velocity"]
    v = c["over"]["erp"] * (0.9286 - root[:, 2]) / 0.002
    below, above = int((v < 0.8 * cap).sum()), int((v > 1.25 * cap).sum())
    print("%-26s erp depth / dt under / over the cap: %d / %d envs (%.3f .. %.3f m/s against %.2f)" % (name, below, above, v.min(), v.max(), cap))
    assert below >= N_ENVS // 8 and above >= N_ENVS // 4, (below, above)


def check_case(name, got_one, got_run, task_const, label=""):
    """Holds a backend's result of a case to the oracle's at the tolerances in this module's docstring; prints the
    measured figures first.  No env is left out of a state comparison."""
    ref_one, ref_run, mu = oracle_run(name, task_const)
    N = N_ENVS
    assert got_one["root_states"].shape == (N, 13) and got_one["dof_state"].shape == (N, 33, 2)
    assert all(np.isfinite(v).all() for v in got_one.values()) and all(np.isfinite(v).all() for v in got_run.values())
    d1, dn = _state_diffs(ref_one, got_one), _state_diffs(ref_run, got_run)
    v32 = _velocity_diff(ref_one, got_one)
    v64 = _velocity_diff(oracle_run(name, task_const, double=True)[0], got_one)
    o3264, bound64 = velocity_bound(name, task_const)
    rel, cone, env = _force_rel(ref_one["contact_forces"], got_one["contact_forces"], mu)
    envs = len(set(env.tolist()))
    pc = lambda x, q: float(np.percentile(x, q)) if len(x) else 0.0
    off_max = float(rel[~cone].max()) if (~cone).any() else 0.0
    print("%-26s %-10s 1 substep: pose %.2e q %.2e v %.2e qd %.2e | velocities vs fp32 %.2e, vs fp64 %.2e (fp32 / fp64 oracles %.2e, bound %.2e) "
          "| forces: %d pairs in %d envs, off cone max %.2e, soles on cone (%d) 50/99/100 %.2e %.2e %.2e | %d substeps: pose %.2e q %.2e v %.2e qd %.2e" % (
              name, label, d1["root pose"], d1["q"], d1["root velocity"], d1["qd"], v32, v64, o3264, bound64, len(rel), envs, off_max,
              int(cone.sum()), pc(rel[cone], 50), pc(rel[cone], 99), pc(rel[cone], 100), RUN_SUBSTEPS, dn["root pose"], dn["q"],
              dn["root velocity"], dn["qd"]))
    assert d1["root pose"] <= STATE_TOL and d1["q"] <= STATE_TOL, (name, d1)
    # velocities: the project bound against the fp32 oracle, or else 4 x the two oracles' own difference against the fp64 one
    assert v32 <= STATE_TOL or v64 <= bound64, (name, v32, v64, bound64)
    if name in NO_CONTACT:
        assert v32 <= STATE_TOL, (name, v32)
    else:
        assert envs >= N // 2, (name, envs)                               # at least half of the envs contribute
    assert off_max <= FORCE_REL, (name, off_max)
    if cone.any():
        assert pc(rel[cone], 50) <= CONE_P50 and pc(rel[cone], 99) <= CONE_P99 and rel[cone].max() <= CONE_MAX, (name, rel[cone].max())
    # bodies the oracle leaves unloaded stay unloaded (within the force tolerance on the largest load of the scene)
    quiet = np.linalg.norm(ref_one["contact_forces"], axis=2) == 0
    scale = max(float(np.abs(ref_one["contact_forces"]).max()), LOADED_N)
    assert np.abs(got_one["contact_forces"][quiet]).max(initial=0.0) <= FORCE_REL * scale, name
    assert dn["root pose"] <= RUN_POS_TOL and dn["q"] <= RUN_POS_TOL, (name, dn)
    assert dn["root velocity"] <= RUN_VEL_TOL and dn["qd"] <= RUN_VEL_TOL, (name, dn)


def check_cone(name, task_const):
    """The oracle's own sliding soles sit on the cone of mu = friction x friction_scale (the check of
    test_sliding_sole_contacts_with_friction_dr_vs_oracle with the plane's coefficient off its default)."""
    one, _, mu = oracle_run(name, task_const)
    cf = one["contact_forces"]
    for foot in _feet():
        f = cf[:, foot]
        loaded = f[:, 2] > LOADED_N
        assert loaded.sum() > N_ENVS // 2
        ratio = np.linalg.norm(f[loaded, :2], axis=1) / f[loaded, 2]
        assert np.all(ratio <= mu[loaded] * 1.02 + 1e-3), name
        if mu.max() > 0:
            assert (ratio > 0.95 * mu[loaded]).mean() > 0.5, name
        else:
            assert np.abs(f[:, :2]).max() == 0.0, name
