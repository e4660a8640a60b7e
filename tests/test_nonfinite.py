"""The step kernels' non-finite guard and the isolation of a bad env's neighbours (tests/nonfinite_cases.py), on the CPU: first
the oracle alone -- it meets every condition by itself -- then the host emulation of the kernel source in its three builds
(tests/emul: KEEP, two-waves, hex).  The GPU tests (tests/test_nonfinite_gpu.py) repeat the scenes through the real library."""
import numpy as np
import pytest

import nonfinite_cases as NF
from emul_backend import EmulSim
from oracle.oracle import OracleSim

BACKENDS = ["oracle", "emul1", "emul2", "emul3"]          # (pytest runs the params in this order: the oracle first)


@pytest.fixture(scope="module")
def makers(task_const):
    def oracle(N, **kw):
        return OracleSim(N, task_const=task_const, **kw)

    def emul(wave_build):
        return lambda N, **kw: EmulSim(N, task_const=task_const, debug_wave_build=wave_build, **kw)

    return {"oracle": oracle, "emul1": emul(1), "emul2": emul(2), "emul3": emul(3)}


@pytest.mark.parametrize("backend", BACKENDS)
def test_every_state_word_poisoned_equals_oracle(makers, backend):
    NF.check_every_word(backend, makers[backend], makers["oracle"])


@pytest.mark.parametrize("scene", NF.PLACEMENT_SCENES, ids=NF.scene_id)
@pytest.mark.parametrize("backend", BACKENDS)
def test_guard_on_the_plane(makers, backend, scene):
    name, place = scene
    buffer, index, value = NF.POISONS[name]
    NF.check_guarded_scene(backend, makers[backend], makers["oracle"], None, [(e, buffer, index, value) for e in NF.PLACEMENTS[place]])


@pytest.mark.parametrize("scene", NF.ACTION_SCENES, ids=NF.scene_id)
@pytest.mark.parametrize("backend", BACKENDS)
def test_non_finite_action_is_clamped(makers, backend, scene):
    NF.check_action_scene(backend, makers[backend], makers["oracle"], *scene)


@pytest.mark.parametrize("scene", NF.TERRAIN_SCENES, ids=NF.scene_id)
@pytest.mark.parametrize("backend", BACKENDS)
def test_guard_on_the_height_field(makers, backend, scene):
    """A NaN / Inf base position on a height field: terrain_sample and terrain_bound must put it on cell 0 (with the clamp written
    as `u < 0 ? 0 : (u > umax ? umax : u)` the NaN passed through and `(int)u` indexed out of the map: a segmentation fault here)."""
    name, env = scene
    NF.check_guarded_scene(backend, makers[backend], makers["oracle"], "slope", [(env, b, i, v) for b, i, v in NF.TERRAIN_POISONS[name]])


@pytest.mark.parametrize("backend", BACKENDS)
def test_guarded_reset_on_a_curriculum_map(makers, backend):
    """Root x NaN on a generated curriculum map: the level the guarded reset moves the env to, its new origin, the level sums and
    dw_terrain_log equal the oracle's."""
    got, ref = NF.check_guarded_scene(backend, makers[backend], makers["oracle"], "curriculum", [(24, "root_states", 0, NF.NAN), (NF.N - 1, "root_states", 1, NF.INF)])
    for g, r in zip(got, ref):
        assert np.array_equal(g["env_origins"][[24, NF.N - 1]], r["env_origins"][[24, NF.N - 1]])
        assert np.array_equal(g["terrain_levels"], r["terrain_levels"]) and np.array_equal(g["level_means"], r["level_means"])
    twin = NF.cached(backend, NF.run_step_scene, makers[backend], "curriculum", 0)
    assert (got[0]["terrain_levels"][[24, NF.N - 1]] != twin[0]["terrain_levels"][[24, NF.N - 1]]).any(), "a guarded reset moves a level"
    assert not np.array_equal(got[1]["level_means"], twin[1]["level_means"]), "and the level sums of the next step show it"


@pytest.mark.parametrize("poison", list(NF.SIMULATE_POISONS))
@pytest.mark.parametrize("kind", [None, "slope"], ids=["plane", "slope"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_simulate_isolates_a_non_finite_env(makers, backend, kind, poison):
    NF.check_simulate_scene(backend, makers[backend], kind, poison)


def test_amp_fused_step_isolates_a_non_finite_env():
    """The fused TocabiAMPLower step (three kernels around dwe_simulate) under the emulation: the 36 envs beside a NaN env are
    bit-identical to the twin run's in every table.  The step has no guard, as the reference: nothing is asserted about the env."""
    NF.check_amp_isolation(NF.run_amp_emul(True), NF.run_amp_emul(False))
