"""The eager-torch twin (oracle/torch_twin.py) against the reference's own functions (live, where the reference
checkout is mounted) and against the committed goldens (everywhere)."""
import os

import numpy as np
import torch

import reference_cases as RC
import replay as R
from isaacgymdyros_amd import abi
from oracle import ref_harness as RH
from oracle import torch_twin as TW


def test_twin_is_bitwise_the_reference_on_cpu(model, task_const):
    """Against the reference's functions' outputs recorded in tests/golden/reference_live.npz (oracle/make_live_goldens.py)
    everywhere, and against the functions themselves where the reference is mounted."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_live.npz"))
    refs = [{k: g[k] for k in g.files if k.startswith("twin/")}]
    if RH.available():
        refs.append(RC.reference_twin(model))
    N = RC.TWIN_N
    d = RC.twin_inputs(N, model)
    nf = model.non_feet_idxs()
    tot, st, r8, qe, col = TW.reward(d["root"], d["target_vel"], d["tq"], d["tf"], d["q"], d["qd"], d["pqd"], d["a"], d["ap"], d["cf"],
                                     d["cfp"][:, model.left_foot_idx], d["cfp"][:, model.right_foot_idx], d["idx"], d["tm"], nf,
                                     model.left_foot_idx, model.right_foot_idx)
    # quaternion helpers
    qa = RC.twin_quat_inputs()
    qd = TW.quat_diff_rad(torch.tensor([[0, 0, 0, 1.0]]).expand(N, 4), qa)
    eul = TW.quat2euler(qa)
    for ref in refs:
        assert torch.equal(tot, torch.from_numpy(ref["twin/total_reward"])) and torch.equal(st, torch.from_numpy(ref["twin/stacked_rewards"]))
        assert torch.equal(r8, torch.from_numpy(ref["twin/crs"]))
        assert int(ref["twin/num_reward_names"]) == 14
        assert torch.equal(qd, torch.from_numpy(ref["twin/quat_diff_rad"]))
        assert len(eul) == 3
        for i, a in enumerate(eul):
            assert torch.equal(a, torch.from_numpy(ref["twin/quat2euler_%d" % i]))


def test_twin_reproduces_the_golden_observations_and_rewards(task_const, model):
    """Goldens were produced by the reference's Python; the twin, fed the golden's injected state and the recorded
    post-step task state, must reproduce the newest observation slot and the rewards bit for bit on the CPU."""
    g = R.load("task_logic_frozen.npz")
    N, steps = int(g["N"]), int(g["steps"])
    mean, var = torch.from_numpy(task_const["obs_mean"]), torch.from_numpy(task_const["obs_var"])
    t = steps - 1
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    # observation: uses post-step (post-reset) state
    obs = TW.observation(T(g["step_root_states"][t]), T(g["step_quat_bias"][t]), T(g["step_qpos_noise"][t]), T(g["step_qpos_bias"][t]),
                         T(g["step_qvel_noise"][t]), T(g["step_time"][t]), T(g["step_init_mocap_data_idx"][t]).long(),
                         T(g["step_target_vel"][t]), T(g["noise"][t][:, abi.K["DW_NZ_VEL"]:abi.K["DW_NZ_VEL"] + 6]), mean, var)
    assert torch.equal(obs, T(g["step_obs_buf"][t][:, 333:370]))
