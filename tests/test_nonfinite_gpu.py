"""The step kernels' non-finite guard and the isolation of a bad env's neighbours on an MI355X: the scenes of tests/nonfinite_cases.py
(each of them passes under the host emulation of the same kernel source first, tests/test_nonfinite.py) through the HIP library in its
three builds and by launch size, then the host class with episode statistics, and the fused TocabiAMPLower step, which has no guard."""
import numpy as np
import pytest
import torch

import nonfinite_cases as NF

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 1, 2, 3], ids=["by_size", "keep", "two_waves", "hex"])
def wave_build(request):
    """DwConfig.debug_wave_build, as the fixture of tests/test_hip_gpu.py: 0 = the build the launch size picks (83 envs: hex), 1 / 2 =
    the KEEP / two-waves octet builds forced, 3 = the hex instantiation forced."""
    return request.param


@pytest.fixture(scope="module")
def oracle_make(task_const):
    from oracle.oracle import OracleSim
    return lambda N, **kw: OracleSim(N, task_const=task_const, **kw)


@pytest.fixture
def hip(task_const, wave_build):
    from hip_backend import HipSim
    return "hip%d" % wave_build, lambda N, **kw: HipSim(N, task_const=task_const, debug_wave_build=wave_build, **kw)


def test_every_state_word_poisoned_equals_oracle(hip, oracle_make):
    NF.check_every_word(hip[0], hip[1], oracle_make, device=True)


@pytest.mark.parametrize("scene", NF.PLACEMENT_SCENES, ids=NF.scene_id)
def test_guard_on_the_plane(hip, oracle_make, scene):
    name, place = scene
    buffer, index, value = NF.POISONS[name]
    NF.check_guarded_scene(hip[0], hip[1], oracle_make, None, [(e, buffer, index, value) for e in NF.PLACEMENTS[place]], device=True)


@pytest.mark.parametrize("scene", NF.ACTION_SCENES, ids=NF.scene_id)
def test_non_finite_action_is_clamped(hip, oracle_make, scene):
    NF.check_action_scene(hip[0], hip[1], oracle_make, *scene)


@pytest.mark.parametrize("scene", NF.TERRAIN_SCENES, ids=NF.scene_id)
def test_guard_on_the_height_field(hip, oracle_make, scene):
    name, env = scene
    NF.check_guarded_scene(hip[0], hip[1], oracle_make, "slope", [(env, b, i, v) for b, i, v in NF.TERRAIN_POISONS[name]], device=True)


def test_guarded_reset_on_a_curriculum_map(hip, oracle_make):
    got, ref = NF.check_guarded_scene(hip[0], hip[1], oracle_make, "curriculum", [(24, "root_states", 0, NF.NAN), (NF.N - 1, "root_states", 1, NF.INF)],
                                      device=True)
    for g, r in zip(got, ref):
        assert np.array_equal(g["env_origins"][[24, NF.N - 1]], r["env_origins"][[24, NF.N - 1]])
        assert np.array_equal(g["terrain_levels"], r["terrain_levels"])
        assert "terrain_log" in g          # (dw_terrain_log against the oracle's level means: check_guarded_scene)


@pytest.mark.parametrize("poison", list(NF.SIMULATE_POISONS))
@pytest.mark.parametrize("kind", [None, "slope"], ids=["plane", "slope"])
def test_simulate_isolates_a_non_finite_env(hip, kind, poison):
    NF.check_simulate_scene(hip[0], hip[1], kind, poison)


def test_host_class_reports_non_finite_joint_and_root_words(wave_build):
    """DyrosDynamicWalk with episode statistics, 83 envs: a NaN joint rate (env 24) and a NaN base x (env N - 1, whose copies pad the
    last wave) end as cause 4, counted twice, and the observations step() returns stay finite."""
    from hip_backend import make_env
    env = make_env(NF.N, episode_stats=True, debug_wave_build=wave_build)
    g = torch.Generator(device="cuda:0").manual_seed(0)
    act = lambda: (torch.rand(NF.N, 13, generator=g, device="cuda:0") * 2 - 1) * 0.3
    for _ in range(3):
        env.step(act())
    nan0 = env.nan_resets.clone()
    env._buf["dof_state"][24, 5, 1] = float("nan")
    env._buf["root_states"][NF.N - 1, 0] = float("nan")
    obs, _r, reset, ex = env.step(act())
    torch.cuda.synchronize()
    cause = ex["termination_cause"].cpu()
    assert int(cause[24]) == 4 and int(cause[NF.N - 1]) == 4
    assert int((cause == 4).sum()) == 2
    d = (env.nan_resets - nan0).view(-1).cpu()
    assert int(d[24]) == 1 and int(d[NF.N - 1]) == 1 and int(d.sum()) == 2
    assert env.episode_stats.summary()["causes"]["non_finite"] == 2
    assert bool(torch.isfinite(obs["obs"]).all())
    assert int(reset[24]) == 1 and int(reset[NF.N - 1]) == 1
    env.close()


@pytest.mark.parametrize("one_launch", [False, True], ids=["three_kernels", "one_launch"])
def test_amp_fused_step_isolates_a_non_finite_env(one_launch):
    """TocabiAMPLower's fused step has no guard (nor has the reference): every table of the fused step and the Gym tensors, for the
    36 envs that share the launch with the NaN env, are bit-identical to the twin run's.  Nothing is asserted about the NaN env."""
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg

    def run(poison):
        cfg = default_amp_cfg(NF.AMP_N, "cuda:0")
        cfg["sim"]["mi355"] = {"amp_fused": True, "amp_one_launch": one_launch, "debug_wave_build": 2}
        env = TocabiAMPLower(cfg, "cuda:0", 0, True)
        g = torch.Generator(device="cuda:0").manual_seed(4)
        for t in range(NF.AMP_STEPS_BEFORE + NF.AMP_STEPS_AFTER):
            env.reset_done()
            if poison and t == NF.AMP_STEPS_BEFORE:
                env._dof_state[NF.AMP_ENV, :, 0] = float("nan")
            env.step((torch.rand(NF.AMP_N, 12, generator=g, device="cuda:0") * 2 - 1) * 0.7)
        torch.cuda.synchronize()
        env._fused_tables()
        out = {n: v.cpu().numpy() for n, v in env._amp_keep.items() if v is not None}
        out.update({"gym_" + k: env._phys._buf[k].cpu().numpy() for k in NF.AMP_GYM})
        env.close()
        return out
    NF.check_amp_isolation(run(True), run(False))
