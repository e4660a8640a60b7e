"""Host logic: the reference's task YAML (Hydra/OmegaConf interpolations, train.py:58-63) resolved without Hydra."""
import json
import os
import pytest

from isaacgymdyros_amd.config import default_cfg, load_task_yaml

SNIPPET = '''
name: DyrosDynamicWalk
physics_engine: ${..physics_engine}
env:
  numEnvs: ${resolve_default:4096,${...num_envs}}
  controlFrequencyInv: 2
sim:
  dt: 0.002
  use_gpu_pipeline: ${eq:${...pipeline},"gpu"}
  physx:
    num_threads: ${....num_threads}
    use_gpu: ${contains:"cuda",${....sim_device}}
    num_subscenes: ${....num_subscenes}
'''


def test_resolvers_follow_the_reference_semantics():
    c = load_task_yaml(SNIPPET)
    assert c["physics_engine"] == "physx" and c["env"]["numEnvs"] == 4096
    assert c["sim"]["use_gpu_pipeline"] is True and c["sim"]["physx"]["use_gpu"] is True
    assert c["sim"]["physx"]["num_threads"] == 4 and c["sim"]["physx"]["num_subscenes"] == 4
    c = load_task_yaml(SNIPPET, num_envs=16384, pipeline="cpu", sim_device="cpu")
    assert c["env"]["numEnvs"] == 16384 and c["sim"]["use_gpu_pipeline"] is False and c["sim"]["physx"]["use_gpu"] is False
    with pytest.raises(KeyError):
        load_task_yaml("a: ${..no_such_key}")


def test_reference_yaml_matches_the_built_in_defaults():
    """Against the reference's task YAML as recorded in tests/golden/reference_cfg.json (oracle/make_live_goldens.py), and
    against the YAML itself where the reference is mounted."""
    import reference_cases as RC
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_cfg.json")) as f:
        ref = json.load(f)["task_yaml"]
    if os.path.exists(RC.task_yaml_path()):
        assert RC.task_yaml_record(RC.task_yaml_path()) == ref
    mine = default_cfg(4096)
    for sec in ("env", "sim"):
        assert ref[sec]
        for k, v in ref[sec].items():
            if k in mine[sec]:
                assert mine[sec][k] == v, (sec, k, mine[sec][k], v)
    assert ref["physx_num_position_iterations"] == mine["sim"]["physx"]["num_position_iterations"]
    assert ref["task_randomize"] == mine["task"]["randomize"]
    ma = mine["task"]["randomization_params"]["actor_params"]["humanoid"]
    assert ref["damping_range"] == ma["dof_properties"]["damping"]["range"]
    assert ref["mass_range"] == ma["rigid_body_properties"]["mass"]["range"]
