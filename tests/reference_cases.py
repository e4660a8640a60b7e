"""The cases the tests that compare with the reference share with oracle/make_live_goldens.py, which records the reference's
answers to them in tests/golden/reference_cfg.json and reference_live.npz: the configurations and seeded inputs, the fields
recorded, and the calls that run them through the reference where it is mounted (oracle/ref_harness.py).  Test helper; importing
it changes nothing."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_terrain.py::test_live_against_reference_when_present
TERRAIN_LIVE = dict(mesh_type="heightfield", curriculum=False, num_rows=2, num_cols=5, border_size=1,
                    terrain_proportions=[0.1, 0.0, 0.2, 0.2, 0.2, 0.1, 0.1])
TERRAIN_SEEDS = (0, 1, 2)
# tests/test_torch_twin.py::test_twin_is_bitwise_the_reference_on_cpu
TWIN_N = 512


def task_yaml_path():
    from oracle import ref_harness
    return os.path.join(ref_harness.IGE, "cfg", "task", "DyrosDynamicWalk.yaml")


def train_yaml_path():
    from oracle import ref_harness
    return os.path.join(ref_harness.IGE, "cfg", "train", "DyrosDynamicWalkPPO.yaml")


def task_yaml_record(path):
    """The fields of the reference's task YAML that the built-in defaults (isaacgymdyros_amd/config.py) must equal."""
    from isaacgymdyros_amd.config import load_task_yaml
    ref = load_task_yaml(path)
    ra = ref["task"]["randomization_params"]["actor_params"]["humanoid"]
    return {"env": {k: v for k, v in ref["env"].items() if not isinstance(v, dict)},
            "sim": {k: v for k, v in ref["sim"].items() if not isinstance(v, dict)},
            "physx_num_position_iterations": ref["sim"]["physx"]["num_position_iterations"],
            "task_randomize": ref["task"]["randomize"],
            "damping_range": ra["dof_properties"]["damping"]["range"],
            "mass_range": ra["rigid_body_properties"]["mass"]["range"]}


def train_yaml_record(path):
    """The `network` and `config` sections of the reference's train YAML (examples/ppo_consumer.py TRAIN_CFG must equal them)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(ROOT, "examples", "ppo_consumer.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    ref = m.load_train_yaml(path)
    return {"network": ref["network"], "config": ref["config"]}


def reference_terrain(seed):
    """Height samples and tile origins of the reference's Terrain for TERRAIN_LIVE and `seed`."""
    import sys
    from oracle import ref_harness
    ref_harness.load_reference(lambda: None)
    ref_terrain, ref_cfg = sys.modules["isaacgymenvs.utils.terrain"], sys.modules["isaacgymenvs.cfg.terrain.terrain_cfg"]
    cfg = ref_cfg.TerrainCfg()
    for k, v in TERRAIN_LIVE.items():
        setattr(cfg, k, v)
    np.random.seed(seed)
    r = ref_terrain.Terrain(cfg, 8)
    return np.asarray(r.heightsamples), np.asarray(r.env_origins)


def twin_inputs(N, model, seed=0):
    """Seeded inputs of the walk reward: root states, contact forces, torques, joint states, actions, mocap indices."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    root = r(N, 13)
    root[:, 3:7] = torch.nn.functional.normalize(r(N, 4) * 0.3 + torch.tensor([0, 0, 0, 1.0]), dim=1)
    cf = torch.zeros(N, 38, 3)
    cf[:, [model.left_foot_idx, model.right_foot_idx], 2] = torch.rand(N, 2, generator=g) * 1500
    cf[::7, 3] = r(len(cf[::7]), 3) * 2
    return dict(root=root, target_vel=torch.rand(N, 2, generator=g), tq=r(N, 33) * 0.3, tf=-torch.rand(N, 2, generator=g) * 600,
                q=r(N, 33) * 0.3, qd=r(N, 33), pqd=r(N, 33), a=torch.rand(N, 13, generator=g) * 2 - 1,
                ap=torch.rand(N, 13, generator=g) * 2 - 1, cf=cf, cfp=cf + r(N, 38, 3) * 20,
                idx=torch.randint(0, 3599, (N, 1), generator=g), tm=100 + torch.rand(N, 1, generator=g) * 10)


def twin_quat_inputs():
    g = torch.Generator().manual_seed(1)
    return torch.nn.functional.normalize(torch.randn(TWIN_N, 4, generator=g), dim=1)


def reference_twin(model):
    """The reference's compute_humanoid_walk_reward, quat_diff_rad and quat2euler on twin_inputs / twin_quat_inputs."""
    from oracle import ref_harness
    mods = ref_harness.load_reference(lambda: None)
    d = twin_inputs(TWIN_N, model)
    nf = model.non_feet_idxs()
    tot, st, names, crs = mods["task"].compute_humanoid_walk_reward(
        torch.zeros(TWIN_N, dtype=torch.long), torch.zeros(TWIN_N, dtype=torch.long), d["target_vel"], d["root"], d["tq"], d["tf"], d["q"],
        torch.zeros(TWIN_N, 33), d["qd"], d["pqd"], d["a"], d["ap"], nf, d["cf"], d["cfp"], d["idx"], 0.6, 0.0, 1.0, d["tm"],
        torch.zeros(TWIN_N), model.right_foot_idx, model.left_foot_idx)
    qa = twin_quat_inputs()
    ident = torch.tensor([[0, 0, 0, 1.0]]).expand(TWIN_N, 4).contiguous()
    out = {"twin/total_reward": tot, "twin/stacked_rewards": st, "twin/crs": crs,
           "twin/quat_diff_rad": mods["jit_utils"].quat_diff_rad(ident, qa)}
    for i, e in enumerate(mods["torch_utils"].quat2euler(qa)):
        out["twin/quat2euler_%d" % i] = e
    out = {k: v.numpy() for k, v in out.items()}
    out["twin/num_reward_names"] = np.asarray(len(names))
    return out
