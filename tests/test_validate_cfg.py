"""Host-side configuration checks (VERDICT r1 weak #5 / ADVICE): every cfg value that becomes a device index or a kernel
size is range-checked by pure Python before the native library is loaded or device memory is allocated, so a bad value
is a ValueError here and never an out-of-range gather on the GPU.  No GPU, no library needed."""
import copy

import pytest

from isaacgymdyros_amd.config import default_cfg, validate_cfg, with_terrain


def test_default_and_terrain_cfgs_pass():
    validate_cfg(default_cfg(64))
    validate_cfg(with_terrain(default_cfg(64), mesh_type="heightfield", curriculum=True, num_rows=10, num_cols=20))
    validate_cfg(with_terrain(default_cfg(8), mesh_type="trimesh", curriculum=False, num_rows=2, num_cols=20))   # N < num_cols is fine


@pytest.mark.parametrize("terrain, msg", [
    (dict(mesh_type="heightfield", curriculum=True, num_rows=2, num_cols=2), "max_init_terrain_level"),   # default 5 >= 2: the r1 abort
    (dict(mesh_type="heightfield", curriculum=True, num_rows=4, num_cols=2, max_init_terrain_level=-1), "max_init_terrain_level"),
    (dict(mesh_type="heightfield", num_rows=0, num_cols=2), "num_rows"),
    (dict(mesh_type="heightfield", num_rows=2, num_cols=0), "num_rows and num_cols"),
    (dict(mesh_type="heightfield", num_rows=2, num_cols=2, terrain_proportions=[0.6, 0.6]), "terrain_proportions"),
    (dict(mesh_type="heightfield", num_rows=2, num_cols=2, terrain_proportions=[-0.1, 0.5]), "terrain_proportions"),
    (dict(mesh_type="heightfield", num_rows=2, num_cols=2, horizontal_scale=0.0), "horizontal_scale"),
    (dict(mesh_type="heightfield", num_rows=2, num_cols=2, terrain_length=8.0, terrain_width=4.0), "square"),
    (dict(mesh_type="heightfield", num_rows=2, num_cols=2, selected=True), "selected"),
    (dict(mesh_type="voxels"), "mesh type"),
])
def test_bad_terrain_cfg_raises_before_any_device_work(terrain, msg):
    cfg = with_terrain(default_cfg(64), **terrain)
    with pytest.raises(ValueError, match=msg):
        validate_cfg(cfg)


def test_bad_env_and_sim_values_raise():
    for path, val, msg in [(("env", "numEnvs"), 0, "numEnvs"), (("env", "numEnvs"), (1 << 20) + 1, "2\\^20"), (("env", "NumHis"), 5, "specialised"),
                           (("env", "controlFrequencyInv"), 4, "controlFrequencyInv"), (("sim", "dt"), 0.0, "dt")]:
        cfg = copy.deepcopy(default_cfg(64))
        cfg[path[0]][path[1]] = val
        with pytest.raises(ValueError, match=msg):
            validate_cfg(cfg)
    cfg = default_cfg(64)
    cfg["sim"]["physx"]["num_position_iterations"] = 100
    with pytest.raises(ValueError, match="iterations"):
        validate_cfg(cfg)


@pytest.mark.parametrize("pos,vel", [(0, 0), (64, 1), (1, 64)])
def test_solver_iteration_sum_outside_1_to_64_is_refused(pos, vel):
    """physx.num_position_iterations + num_velocity_iterations becomes DwConfig.solver_iterations: 0 and 65 are refused, the
    ends of the range pass."""
    cfg = default_cfg(64)
    cfg["sim"]["physx"].update(num_position_iterations=pos, num_velocity_iterations=vel)
    with pytest.raises(ValueError, match="iterations"):
        validate_cfg(cfg)
    for ok in ((1, 0), (63, 1)):
        cfg["sim"]["physx"].update(num_position_iterations=ok[0], num_velocity_iterations=ok[1])
        validate_cfg(cfg)


def test_amp_body_states_is_checked_like_the_other_amp_keys():
    """validate_cfg checks sim.mi355.amp_body_states as it checks body_states and the other amp_* keys of the model tensors: the ValueError
    is body_states.validate's, which TocabiAMPLower raises for the same cfg."""
    from isaacgymdyros_amd import body_states
    cfg = default_cfg(64)
    cfg["sim"]["mi355"]["amp_body_states"] = {"bodies": ["Head_Link", "L_Foot_Link", "R_Foot_Link"]}
    validate_cfg(cfg)
    for bad in ({"bodies": ["Head"]}, {"mass": True}, {"com": 1}, "on"):
        with pytest.raises(ValueError) as want:
            body_states.validate(bad)
        cfg["sim"]["mi355"]["amp_body_states"] = bad
        with pytest.raises(ValueError) as got:
            validate_cfg(cfg)
        assert str(got.value) == str(want.value)


def test_constructor_validates_before_touching_the_library(monkeypatch):
    """The task constructor must fail on the cfg check, not on library loading / allocation: make loading the library
    an error and see the ValueError of the cfg instead."""
    from isaacgymdyros_amd import _lib
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk

    def boom():
        raise AssertionError("library loaded before the configuration was validated")
    monkeypatch.setattr(_lib, "load", boom)
    cfg = with_terrain(default_cfg(64), mesh_type="heightfield", curriculum=True, num_rows=2, num_cols=2)
    with pytest.raises(ValueError, match="max_init_terrain_level"):
        DyrosDynamicWalk(cfg, "cuda:0", 0, True)
