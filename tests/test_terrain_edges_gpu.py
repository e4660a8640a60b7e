"""The height-field instantiation of the step kernels on the MI355X: the hand-made scenes of tests/terrain_edge_cases.py (map edges,
sample and bound-cell lines, other grid scales, pillars only the reach window of the bound table knows, fallen robots at the outline)
against the oracle on every build, and generated terrain at the launch sizes where the builds are chosen (S = 4 x CUs: hex up to 4 S,
KEEP up to 8 S, two waves above).  tests/test_terrain_edges.py holds on the CPU that the scenes reach what they are named for."""
import numpy as np
import pytest
import torch

import terrain_edge_cases as TE
from test_hip_gpu import _STEP_BUFFERS, _device_simds, _dr_rollout_buffers

pytestmark = pytest.mark.gpu

# the curriculum map of test_terrain_checkpoint_and_reset_done
TDICT = dict(mesh_type="heightfield", curriculum=True, num_rows=4, num_cols=5, border_size=2, max_init_terrain_level=3)
# the map of test_terrain_physics_vs_oracle_on_gpu
WALK_TDICT = dict(mesh_type="heightfield", curriculum=True, num_rows=2, num_cols=4, border_size=2, max_init_terrain_level=1,
                  terrain_proportions=[0.2, 0.2, 0.3, 0.3, 0.0])


@pytest.mark.parametrize("wave_build", [0, 1, 2, 3], ids=["by_size", "keep", "two_waves", "hex"])
@pytest.mark.parametrize("name", list(TE.SCENES))
def test_edge_scene_vs_oracle(name, wave_build):
    """One substep of every scene through dw_simulate of the HIP library, each build, at the tolerances of
    tests/terrain_edge_cases.py (loaded bodies, forces, positions 1e-5, velocities 1e-5 or 4 x the two oracles' own difference)."""
    from hip_backend import HipSim
    got = TE.run_scene(lambda N, terrain: HipSim(N, terrain=terrain, terrain_curriculum=0, debug_wave_build=wave_build), name)
    TE.check(name, got, label="hip wb%d" % wave_build)


def test_keep_and_two_waves_builds_agree_bitwise_on_terrain():
    """The terrain twin of test_keep_and_two_waves_builds_agree_bitwise: at 4 S + 1 envs on a generated curriculum map, 10 steps with DR
    and random actions, the two forms of the octet kernels leave the same bits (scratch in use at full occupancy in one of them, the
    last workgroup's second wave empty in both)."""
    N = 4 * _device_simds() + 1
    keep, two = _dr_rollout_buffers(N, 1, terrain=TDICT), _dr_rollout_buffers(N, 2, terrain=TDICT)
    assert float(keep["root_states"][:, 2].std()) > 0.05          # (the robots stand at their tiles' heights: not the plane)
    for key in _STEP_BUFFERS:
        assert torch.equal(keep[key], two[key]), key


@pytest.mark.parametrize("k,extra,expect,other", [(4, 0, 3, 1), (4, 1, 1, 3), (8, 0, 1, 3), (8, 1, 2, 3)], ids=["4S", "4S+1", "8S", "8S+1"])
def test_launch_size_picks_the_build_on_terrain(k, extra, expect, other):
    """The terrain twin of test_launch_size_picks_the_build: on each side of both thresholds the by-size rollout on the curriculum map
    equals the build it should select bit for bit and differs from the other layout's."""
    N = k * _device_simds() + extra
    got, want, nope = (_dr_rollout_buffers(N, wb, terrain=TDICT) for wb in (0, expect, other))
    for key in _STEP_BUFFERS:
        assert torch.equal(got[key], want[key]), (N, key)
    assert not torch.equal(got["dof_state"], nope["dof_state"]), N


@pytest.mark.parametrize("k", [4, 8], ids=["4S+1", "8S+1"])
def test_walking_range_substep_vs_oracle_at_the_build_sizes(k):
    """The walking-range scene of test_terrain_physics_vs_oracle_on_gpu drawn for N = 4 S + 1 (the smallest KEEP launch) and 8 S + 1
    (the smallest two-waves launch), build chosen by size, one substep, at the checks of tests/terrain_edge_cases.py with the fp64
    rule for the velocities (not the load-scaled bound of that test, which was measured at 256 envs)."""
    from hip_backend import make_env
    from isaacgymdyros_amd.terrain import Terrain, TerrainCfg
    from oracle.oracle import OracleSim
    N = k * _device_simds() + 1
    env = make_env(N, randomize=False, terrain=WALK_TDICT, seed=3, debug_wave_build=0)
    t = Terrain(TerrainCfg(**WALK_TDICT), N, seed=3)
    assert np.array_equal(env.height_samples.cpu().numpy(), t.heightsamples)
    rng = np.random.default_rng(5)
    root, dof = np.zeros((N, 13), np.float32), np.zeros((N, 33, 2), np.float32)
    org = t.env_origins.reshape(-1, 3)[rng.integers(0, 8, size=N)]
    root[:, 0:2] = org[:, 0:2] + rng.uniform(-3, 3, size=(N, 2))
    root[:, 2] = t.height_at(root[:, 0], root[:, 1]) + 0.93 + rng.uniform(-0.03, 0.05, size=N)
    root[:, 6] = 1.0
    root[:, 7:13] = rng.normal(size=(N, 6)) * 0.3
    dof[:, :, 0] = np.asarray(TE.Q0) + rng.normal(size=(N, 33)) * 0.05
    dof[:, :, 1] = rng.normal(size=(N, 33)) * 0.5
    tau = rng.uniform(-30, 30, size=(N, 33)).astype(np.float32)
    refs = []
    for double in (False, True):
        A = OracleSim(N, terrain=t, double=double)
        A.buf["root_states"][...], A.buf["dof_state"][...] = root, dof
        A.simulate(tau)
        refs.append({key: A.buf[key].copy() for key in ("root_states", "dof_state", "contact_forces")})
    env.root_states.copy_(torch.from_numpy(root).cuda())
    env._buf["dof_state"].copy_(torch.from_numpy(dof).cuda())
    env.simulate(torch.from_numpy(tau).cuda()); torch.cuda.synchronize()
    got = {"root_states": env.root_states.cpu().numpy(), "dof_state": env._buf["dof_state"].cpu().numpy(), "contact_forces": env.contact_forces.cpu().numpy()}
    env.close()
    c = TE.compare(refs[0], refs[1], got)
    print("walking range, %d envs by size:" % N, c)
    assert (np.linalg.norm(refs[0]["contact_forces"], axis=2).max(axis=1) > 100.0).sum() > N // 2          # the terrain is being touched
    assert c["finite"] and c["loaded_mismatch"] == 0 and c["force"] <= c["force_tol"], c
    assert c["pos"] <= TE.STATE_TOL, c
    assert c["v32"] <= TE.STATE_TOL or c["v64"] <= c["v64_bound"], c


def test_ten_policy_steps_vs_both_oracles_at_8s_plus_1_on_terrain(task_const):
    """Ten policy steps with DR and random actions on the curriculum map at 8 S + 1 envs (the smallest two-waves launch, its last
    workgroup's second wave empty), build by size, against the fp32 oracle -- with bounds that come from the oracles: the fp64 oracle
    runs the same rollout, and the kernels' per-env worst |dq|, |dqd| and root pose difference from the fp32 oracle is held, at the
    50th and the 99th percentile of the envs, to 4 x the same percentile of the fp32-to-fp64 oracle difference.  An env whose reset
    flag differs leaves its comparison (kernel / fp32 oracle, and fp32 / fp64 oracle, each on its own); at least 98 % must stay in the
    first (the flat test's 16 per 2048) and, as the condition that the map is not too rough for the bound to mean anything, at least
    99 % in the second.  Reset-time draws, terrain levels and env origins of the envs that stay are bit-identical.

    The map (4 levels x 5 types, every starting level) meets the condition: on the CPU, with a stand-in initial state drawn in numpy
    (robots on their tiles, friction and damping DR), the two oracles disagreed on 0 reset flags of 8193 envs in 10 steps (|dq| 4.5e-7 /
    1.1e-6 at the 50th / 99th percentile); on the MI355X, from the env's own initial state, 0 of 8193 for the oracles and 0 for the
    kernels, |dq| 4.5e-6 / 6.0e-5 against the oracles' 4.1e-6 / 6.0e-5, |dqd| 6.8e-4 / 1.5e-2 against 6.1e-4 / 1.5e-2, root pose 8.3e-7 /
    1.3e-5 against 3.8e-6 / 1.5e-5."""
    from hip_backend import make_env
    from oracle.oracle import OracleSim
    N = 8 * _device_simds() + 1
    env = make_env(N, debug_wave_build=0, friction_dr=True, seed=21, terrain=TDICT)
    oras = []
    for double in (False, True):
        o = OracleSim(N, task_const=task_const, cfg=env._ccfg, terrain=env.terrain, double=double)
        for key, t in env._buf.items():
            o.buf[key][...] = t.cpu().numpy().reshape(o.buf[key].shape)
        oras.append(o)
    o32, o64 = oras
    g = torch.Generator().manual_seed(8)
    alive = {"kernel": np.ones(N, bool), "oracles": np.ones(N, bool)}
    worst = {who: {k: np.zeros(N) for k in ("dq", "dqd", "root")} for who in alive}
    for t in range(10):
        a = torch.rand(N, 13, generator=g) * 2 - 1
        env.step(a.cuda())
        o32.step(a.numpy(), None, t); o64.step(a.numpy(), None, t)
        torch.cuda.synchronize()
        got = {"reset_buf": env.reset_buf.cpu().numpy(), "dof_state": env._buf["dof_state"].cpu().numpy(), "root_states": env.root_states.cpu().numpy()}
        for who, (x, y) in (("kernel", (got, o32.buf)), ("oracles", (o64.buf, o32.buf))):
            alive[who] &= x["reset_buf"] == y["reset_buf"]
            cmp = alive[who] & (o32.buf["reset_buf"] == 0)
            w = worst[who]
            w["dq"][cmp] = np.maximum(w["dq"][cmp], np.abs(x["dof_state"][cmp, :, 0] - y["dof_state"][cmp, :, 0]).max(axis=1))
            w["dqd"][cmp] = np.maximum(w["dqd"][cmp], np.abs(x["dof_state"][cmp, :, 1] - y["dof_state"][cmp, :, 1]).max(axis=1))
            w["root"][cmp] = np.maximum(w["root"][cmp], np.abs(x["root_states"][cmp, :7] - y["root_states"][cmp, :7]).max(axis=1))
    pct = {who: {k: [float(np.percentile(v[alive[who]], p)) for p in (50, 99)] for k, v in w.items()} for who, w in worst.items()}
    left = {who: int(N - m.sum()) for who, m in alive.items()}
    print("%d envs on terrain, 10 steps, per-env worst, percentiles 50 / 99:" % N, pct, "left the comparison:", left)
    assert float(np.ptp(o32.buf["env_origins"][:, 2])) > 0.05                       # (tiles at different heights: not the plane)
    assert left["oracles"] <= 0.01 * N, left
    assert left["kernel"] <= 0.02 * N, left
    for k in ("dq", "dqd", "root"):
        for i in (0, 1):
            assert pct["kernel"][k][i] <= 4.0 * pct["oracles"][k][i], (k, (50, 99)[i], pct)
    stay = alive["kernel"]
    for k in ("dof_damping", "dof_armature", "friction_scale", "terrain_levels", "env_origins"):
        assert np.array_equal(env._buf[k].cpu().numpy().reshape(o32.buf[k].shape)[stay], o32.buf[k][stay]), k
    env.close()
