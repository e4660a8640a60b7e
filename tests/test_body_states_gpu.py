"""The rigid-body state tensor on an MI355X (include/dyros_bodies.h, csrc/dw_bodies.hip): the HIP kernel against the
float64 restatement of tests/body_states_ref.py under its measured tolerance at the workgroup's edges, with the output buffers too long and
their tails watched; the ways to choose outputs; agreement with dw_body_positions; a live env with resets; a captured step plus refresh; and
TocabiAMPLower's maintained rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import body_states_ref as R
from isaacgymdyros_amd import body_states as B
from isaacgymdyros_amd.model import load_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = B.GROUP          # envs per workgroup
PAD, SENTINEL = 64, -7.25
SUBSET = [37, 0, 16, 8, 8]


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def api():
    return B.declare(__import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0])


@pytest.fixture(scope="module")
def table(api):
    return torch.from_numpy(B.pack_table(api, load_model()).view(np.int32)).to(DEV)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def refresh(api, table, root, dof, ms, vel_at_com, ids=None, states=True, com=True, expect=0):
    """dwb_refresh on numpy inputs; the outputs are PAD words too long and filled with SENTINEL, and every word past the end must come back
    untouched.  Returns (states [n, nb, 13], com [n, 7]) as numpy arrays (None where not asked for)."""
    n, nb = len(root), 38 if ids is None else len(ids)
    d = [dev(root), dev(dof), dev(ms)]
    st = torch.full((n * nb * 13 + PAD,), SENTINEL, device=DEV) if states else None
    cm = torch.full((n * 7 + PAD,), SENTINEL, device=DEV) if com else None
    arr = None if ids is None else (C.c_int32 * nb)(*ids)
    rc = api["refresh"](n, table.data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), arr, 0 if ids is None else nb, vel_at_com, ptr(st), ptr(cm), stream())
    torch.cuda.synchronize()          # (d is freed after this)
    assert rc == expect, api["last_error"]()
    out = []
    for t, words in ((st, n * nb * 13), (cm, n * 7)):
        if t is None:
            out.append(None)
            continue
        h = t.cpu().numpy()
        assert (h[words:] == np.float32(SENTINEL)).all(), np.argwhere(h[words:] != np.float32(SENTINEL))[:5]
        out.append(h[:words] if rc == 0 else h)
    if rc != 0:
        return out
    return out[0].reshape(n, nb, 13) if states else None, out[1].reshape(n, 7) if com else None


# ---------------------------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("n", [1, G - 1, G, G + 1, 3 * G + 5])
def test_kernel_against_float64(api, table, n, vel_at_com):
    """n = 1: one env in one workgroup; G - 1, G, G + 1: the group's edge; 3 G + 5: three whole groups and a partial one."""
    root, dof, ms = R.states(n, 100 * n + vel_at_com, mass=True)
    st, cm = refresh(api, table, root, dof, ms, vel_at_com)
    ex = R.excess(st, cm, root, dof, ms, vel_at_com, report="gpu n=%d vel_at_com=%d" % (n, vel_at_com))
    assert R.within(ex), ex
    assert np.array_equal(st[:, 0].view(np.uint32), root.view(np.uint32))          # row 0 is the root row, bit for bit
    u = st.view(np.uint32)
    for carrier, welded in ((6, (7, 8)), (14, (15, 16))):
        for g in welded:
            assert np.array_equal(u[:, g, 0:7], u[:, carrier, 0:7]) and np.array_equal(u[:, g, 10:13], u[:, carrier, 10:13])


def test_kernel_640_m_out(api, table):
    """Base x, y uniform in +-640 m, where the 16384-env grid puts its last envs: the offsets are as accurate as at the origin."""
    n = 3 * G + 5
    root, dof, ms = R.states(n, 7, xy=640.0, mass=True)
    st, cm = refresh(api, table, root, dof, ms, 1)
    ex = R.excess(st, cm, root, dof, ms, 1, report="gpu 640 m")
    assert R.within(ex), ex


# ---------------------------------------------------------------------------------------------- output selection
def test_output_selection(api, table):
    n = 2 * G + 3
    root, dof, ms = R.states(n, 8, mass=True)
    full, com = refresh(api, table, root, dof, ms, 1)
    st, none = refresh(api, table, root, dof, ms, 1, com=False)
    assert none is None and np.array_equal(st.view(np.uint32), full.view(np.uint32))
    none, cm = refresh(api, table, root, dof, ms, 1, states=False)
    assert none is None and np.array_equal(cm.view(np.uint32), com.view(np.uint32))
    one, _ = refresh(api, table, root, dof, ms, 1, ids=[29])
    assert one.shape == (n, 1, 13) and np.array_equal(one.view(np.uint32), full[:, [29]].view(np.uint32))
    sub, cm = refresh(api, table, root, dof, ms, 1, ids=SUBSET)          # (5 * 13 words per env: the group's block is written in 16-byte pieces and a tail)
    assert np.array_equal(sub.view(np.uint32), full[:, SUBSET].view(np.uint32)) and np.array_equal(cm.view(np.uint32), com.view(np.uint32))
    # no mass scale: the nominal masses
    _, cm1 = refresh(api, table, root, dof, None, 1, states=False)
    assert R.within(R.excess(None, cm1, root, dof, None, 1))
    # an id of 38 is refused, and nothing was launched: both buffers still hold the sentinel
    st, cm = refresh(api, table, root, dof, ms, 1, ids=[0, 38], expect=-1)
    assert b"outside 0..37" in api["last_error"]() and (st == np.float32(SENTINEL)).all() and (cm == np.float32(SENTINEL)).all()


def test_an_unaligned_states_pointer_takes_the_word_path(api, table):
    """`states` 4 bytes past a 16-byte boundary: the same bits, written word by word."""
    n = G + 3
    root, dof, ms = R.states(n, 9)
    full, _ = refresh(api, table, root, dof, ms, 0, com=False)
    d = [dev(root), dev(dof)]
    buf = torch.full((1 + n * 38 * 13 + PAD,), SENTINEL, device=DEV)
    assert buf.data_ptr() % 16 == 0
    assert api["refresh"](n, table.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), None, None, 0, 0, buf.data_ptr() + 4, None, stream()) == 0
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert h[0] == np.float32(SENTINEL) and (h[1 + n * 494:] == np.float32(SENTINEL)).all()
    assert np.array_equal(h[1:1 + n * 494].view(np.uint32), full.reshape(-1).view(np.uint32))


# ---------------------------------------------------------------------------------------------- envs
def make_env(n, spec=None, **mi):
    from isaacgymdyros_amd.config import default_cfg
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = default_cfg(n, DEV)
    cfg["seed"] = 42
    cfg["env"]["episodeLength"] = 0.1          # (seconds; 0.004 s per policy step: every env meets the time limit at step 25)
    cfg["sim"]["mi355"]["device_step_counter"] = True
    cfg["sim"]["mi355"]["alias_obs"] = True
    cfg["sim"]["mi355"].update(mi)
    if spec is not None:
        cfg["sim"]["mi355"]["body_states"] = spec
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def actions(n, steps, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    amp = torch.tensor([0.0, 0.05, 0.3, 1.0], device=DEV)[torch.arange(n, device=DEV) % 4].view(1, n, 1)
    return ((torch.rand(steps, n, 13, generator=g, device=DEV) * 2 - 1) * amp).contiguous()


def test_agrees_with_dw_body_positions(api, table):
    """Rows of the Gym bodies of moving bodies [6, 12, 0, 3, 22, 33, 15, 30] against dw_body_positions on +-1 m bases: 5e-6 m, the bound of
    tests/test_amp_gpu.py test_body_positions_hip_vs_oracle."""
    n = 64
    env = make_env(n, True)
    root, dof, _ = R.states(n, 10)
    env._buf["root_states"].copy_(torch.from_numpy(root))
    env._buf["dof_state"].copy_(torch.from_numpy(dof))
    moving = [6, 12, 0, 3, 22, 33, 15, 30]
    arr = (C.c_int32 * len(moving))(*moving)
    out = torch.zeros(n, len(moving), 3, device=DEV)
    assert env._api["body_positions"](env._h, arr, len(moving), C.c_void_p(out.data_ptr()), None) == 0
    st = env.refresh_rigid_body_state_tensor()
    assert st is env.body_states.states
    gym = [load_model().mv_gym[m] for m in moving]
    err = float((st[:, gym, 0:3] - out).abs().max())
    print("against dw_body_positions: %.2e m" % err)
    env.close()
    assert err < 5e-6


def bits(*ts):
    return torch.cat([t.reshape(-1).view(torch.int32) if t.dtype == torch.float32 else t.reshape(-1).to(torch.int32) for t in ts])


def test_live_env_with_resets(api, table):
    n, steps = 64, 40
    acts = actions(n, steps)
    runs = {}
    for name, spec, mi in (("off", None, {}), ("auto", {"auto": True}, {}),
                           ("subset", {"bodies": ["Head_Link", "L_Foot_Link", "R_Foot_Link"], "com": False, "auto": True}, {"episode_stats": True})):
        env = make_env(n, spec, **mi)
        a, h, resets = torch.zeros(n, 13, device=DEV), [], 0
        if spec is None:
            assert env.body_states is None
            with pytest.raises(RuntimeError):
                env.refresh_rigid_body_state_tensor()
        for i in range(steps):
            a.copy_(acts[i])
            o, r, d, _ex = env.step(a)
            h.append(bits(o["obs"], r, d, env._buf["root_states"]))
            resets += int(d.sum())
            if name == "auto":
                bs = env.body_states
                held = bs.states.clone(), bs.com.clone()
                b = env._buf
                root, dof, ms = (b[k].cpu().numpy() for k in ("root_states", "dof_state", "mass_scale"))
                st, cm = refresh(api, table, root, dof, ms, bs.vel_at_com)
                assert np.array_equal(held[0].cpu().numpy().view(np.uint32), st.view(np.uint32)), i
                assert np.array_equal(held[1].cpu().numpy().view(np.uint32), cm.view(np.uint32)), i
                if i % 13 == 0 or i == steps - 1:
                    ex = R.excess(st, cm, root, dof, ms, bs.vel_at_com)
                    assert R.within(ex), (i, ex)
        if name == "auto":
            assert bs.vel_at_com == 1 and bs.names == load_model().body_names and bs.parents == load_model().body_parent
            assert bs.pos.shape == (n, 38, 3) and bs.rot.shape == (n, 38, 4) and bs.vel.shape == (n, 38, 3) and bs.ang_vel.shape == (n, 38, 3)
            assert bs.index("Head_Link") == 29 and torch.equal(bs.rows("R_Foot_Link", "Head_Link"), bs.states[:, [16, 29]])
            # reset_idx refreshes too
            env.reset_idx(torch.arange(0, n, 2, device=DEV))
            assert torch.equal(bs.states[:, 0], env._buf["root_states"])
        if name == "subset":
            bs = env.body_states
            assert bs.com is None and bs.names == ["Head_Link", "L_Foot_Link", "R_Foot_Link"] and bs.parents == [-1, -1, -1] and bs.ids == [29, 8, 16]
            assert bs.states.shape == (n, 3, 13)
        runs[name] = torch.stack(h).cpu()
        env.close()
        assert resets > 0          # (the time limit alone resets every env)
    # the feature only reads: the same bits with the key absent, on, and on beside another recorder in a rebuilt env
    assert torch.equal(runs["off"], runs["auto"]) and torch.equal(runs["off"], runs["subset"])


def test_captured_step_plus_refresh_replays_the_eager_bits():
    """Step and refresh recorded in one graph on one stream (a linear chain), replayed 10 times, against 10 eager steps from the same state."""
    n = 64
    acts = actions(n, 11, seed=3)
    outs = []
    for captured in (False, True):
        env = make_env(n, {"auto": True})
        a = torch.zeros(n, 13, device=DEV)
        a.copy_(acts[0])
        env.step(a)                            # (the first step is eager on both sides)
        torch.cuda.synchronize()
        h = []
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            a.copy_(acts[1])
            with torch.cuda.graph(g, stream=side):
                env.step(a)
            # (the capture itself ran nothing: replay the recorded step for each of the 10 actions)
        for i in range(1, 11):
            a.copy_(acts[i])
            if captured:
                g.replay()
            else:
                env.step(a)
            h.append(bits(env.body_states.states, env.body_states.com, env._buf["root_states"]))
        torch.cuda.synchronize()
        outs.append(torch.stack(h).cpu())
        env.close()
    assert torch.equal(outs[0], outs[1])


def test_tocabi_amp_lower_rows():
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    n = 64
    cfg = default_amp_cfg(n, DEV)
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert amp.body_states is None
    with pytest.raises(RuntimeError):
        amp.refresh_rigid_body_state_tensor()
    amp.close()
    cfg = default_amp_cfg(n, DEV)
    cfg["sim"].setdefault("mi355", {})["amp_body_states"] = True
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert isinstance(amp.body_states, B.BodyStates) and amp._phys.body_states is None
    assert amp.body_states.vel_at_com == int(amp._phys._ccfg.root_vel_at_com)
    g = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(20):
        amp.step((torch.rand(n, amp.num_actions, generator=g, device=DEV) * 2 - 1) * 0.1)
    amp.refresh_rigid_body_state_tensor()
    err = float((amp.body_states.pos[:, [0, 8, 16]] - amp._rigid_body_pos[:, [0, 8, 16]]).abs().max())
    print("against TocabiAMPLower's maintained rows: %.2e m" % err)
    moved = float((amp._rigid_body_pos[:, 8] - amp._rigid_body_pos[:, 16]).abs().max())
    amp.close()
    assert err < 5e-6 and moved > 0.1


# ---------------------------------------------------------------------------------------------- the player
def test_player_writes_the_body_trajectories(tmp_path):
    import importlib.util
    import os
    import subprocess
    import sys
    from isaacgymdyros_amd import ppo_checkpoint as PK
    from isaacgymdyros_amd import ppo_update as U
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(root, "examples", "ppo_consumer.py"))
    ppo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ppo)
    torch.manual_seed(3)
    net = ppo.DyrosActorCritic(U.IN, U.ACT, ppo.TRAIN_CFG["network"]).to(DEV)          # an untrained policy
    c = ppo.TRAIN_CFG["config"]
    ck = PK.save(str(tmp_path / "p.pth"), net, epoch=0, opt_actor=torch.optim.Adam(net.actor_parameters(), lr=c["learning_rate"]),
                 opt_critic=torch.optim.Adam(net.critic_parameters(), lr=c["critic_lr"]))
    out = tmp_path / "bodies"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "examples", "ppo_player.py"), "--checkpoint", ck, "--num-envs", "64",
                        "--games", "64", "--max-steps", "60", "--episode-length", "0.1", "--bodies-dir", str(out), "--bodies-envs", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["bodies_env0.npz", "bodies_env1.npz"]
    z = np.load(out / "bodies_env1.npz")
    T = z["states"].shape[0]
    assert 20 <= T <= 60 and z["states"].shape == (T, 38, 13) and z["com"].shape == (T, 7) and float(z["dt"]) == pytest.approx(0.004)
    assert z["names"].tolist() == load_model().body_names and z["parents"].tolist() == load_model().body_parent
    assert np.isfinite(z["states"]).all() and np.abs(np.linalg.norm(z["states"][..., 3:7], axis=-1) - 1).max() < 1e-5
    # a child's origin stays at its link length from its parent's: the rows are one robot's
    d = np.linalg.norm(z["states"][:, 4, 0:3] - z["states"][:, 3, 0:3], axis=-1)
    assert d.max() - d.min() < 1e-5 and d.min() > 0.1
