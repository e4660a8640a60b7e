"""The Jacobian and mass-matrix tensors on an MI355X (include/dyros_jacobians.h, csrc/dw_jacobian.hip): the HIP kernels
against the float64 reference of tests/jacobians_ref.py under its measured tolerance at the workgroup's edges, with the output buffers filled
with NaN, too long, and their tails watched; the outputs' exact properties; the ways to choose outputs; an unaligned output; agreement with
dwb_refresh's own velocities; a live env with resets; a captured step plus both refreshes; TocabiAMPLower; the player's files."""
import ctypes as C

import numpy as np
import pytest
import torch

import body_states_ref as R
import jacobians_ref as JR
from isaacgymdyros_amd import body_states as B
from isaacgymdyros_amd import jacobians as JM
from isaacgymdyros_amd.model import load_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = JM.GROUP          # envs per workgroup, both kernels
PAD = 64
SUBSET = [37, 0, 16, 8, 8]
F, U = np.float32, np.uint32


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def api():
    return JM.declare(__import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0])


@pytest.fixture(scope="module")
def table(api):
    return torch.from_numpy(JM.pack_table(api, load_model()).view(np.int32)).to(DEV)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def nan_buffer(words, offset=0):
    return torch.full((offset + words + PAD,), float("nan"), device=DEV)


def taken(buf, words, offset=0, finite=True):
    """The first `words` words of a NaN-filled buffer after a launch: every one written (when the inputs were finite), none beyond."""
    h = buf.cpu().numpy()
    assert np.isnan(h[:offset]).all() and np.isnan(h[offset + words:]).all(), "a word outside the output was written"
    out = h[offset:offset + words]
    if finite:
        assert np.isfinite(out).all(), "%d words were not written" % int(np.isnan(out).sum())
    return out.copy()


def jac(api, table, root, dof, vel_at_com, ids=None, expect=0, finite=True):
    n, nb = len(root), 38 if ids is None else len(ids)
    d = [dev(root), dev(dof)]
    out = nan_buffer(n * nb * 234)
    arr = None if ids is None else (C.c_int32 * nb)(*ids)
    rc = api["jacobian"](n, table.data_ptr(), ptr(d[0]), ptr(d[1]), arr, 0 if ids is None else nb, vel_at_com, ptr(out), stream())
    torch.cuda.synchronize()          # (d is freed after this)
    assert rc == expect, api["last_error"]()
    if rc != 0:
        assert np.isnan(out.cpu().numpy()).all()          # nothing was launched
        return None
    return taken(out, n * nb * 234, finite=finite).reshape(n, nb, 6, 39)


def mm(api, table, root, dof, ms, arm, vel_at_com, cj=True, finite=True):
    n = len(root)
    d = [dev(root), dev(dof), dev(ms), dev(arm)]
    out, oc = nan_buffer(n * 1521), nan_buffer(n * 117) if cj else None
    rc = api["mass_matrix"](n, table.data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), vel_at_com, ptr(out), ptr(oc), stream())
    torch.cuda.synchronize()
    assert rc == 0, api["last_error"]()
    return taken(out, n * 1521, finite=finite).reshape(n, 39, 39), taken(oc, n * 117, finite=finite).reshape(n, 3, 39) if cj else None


# ---------------------------------------------------------------------------------------------- the kernels against float64
@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("n", [1, G - 1, G, G + 1, 3 * G + 5])
def test_kernels_against_float64(api, table, n, vel_at_com):
    """n = 1: one env in one workgroup; G - 1, G, G + 1: the group's edge; 3 G + 5: three whole groups and a partial one."""
    root, dof, ms = R.states(n, 100 * n + vel_at_com, mass=True)
    arm = JR.armature_of(n, n)
    J = jac(api, table, root, dof, vel_at_com)
    M, CJ = mm(api, table, root, dof, ms, arm, vel_at_com)
    ex = JR.excess(root, dof, ms, arm, vel_at_com, J, M, CJ, report="gpu n=%d vel_at_com=%d" % (n, vel_at_com))
    assert JR.within(ex), ex
    exact_properties(J, M, CJ)


def exact_properties(J, M, CJ):
    n = len(J)
    assert np.array_equal(M.view(U), np.swapaxes(M, 1, 2).view(U))                                             # symmetric bit for bit
    mask = np.broadcast_to(JR.dof_mask()[:, None, :], (38, 6, 39))
    assert (J.view(U)[:, ~mask] == 0).all() and (M.view(U)[:, ~JR.branch_mask()] == 0).all()              # +0.0, not -0.0
    eye = np.zeros((6, 39), F)
    eye[np.arange(6), np.arange(6)] = 1
    assert np.array_equal(J[:, 0].view(U), np.broadcast_to(eye, (n, 6, 39)).view(U))                         # row 0 is [I 0; 0 I | 0]
    assert np.array_equal(J[:, :, 0:3, 0:3].view(U), np.broadcast_to(eye[0:3, 0:3], (n, 38, 3, 3)).view(U))
    assert np.array_equal(J[:, :, 3:6, 0:6].view(U), np.broadcast_to(eye[3:6, 0:6], (n, 38, 3, 6)).view(U))
    assert (J[:, :, [0, 1, 2], [3, 4, 5]].view(U) == 0).all()
    if CJ is not None:
        assert np.array_equal(CJ[:, :, 0:3].view(U), np.broadcast_to(eye[0:3, 0:3], (n, 3, 3)).view(U))


def test_exact_properties_subset_far_and_nan(api, table):
    n = 2 * G + 3
    root, dof, ms = R.states(n, 8, mass=True)
    arm = JR.armature_of(n, 9)
    J, (M, CJ) = jac(api, table, root, dof, 1), mm(api, table, root, dof, ms, arm, 1)
    # a subset with a repeat (5 * 234 words per env), and one body: the full tensor's rows bit for bit
    sub = jac(api, table, root, dof, 1, ids=SUBSET)
    assert np.array_equal(sub.view(U), J[:, SUBSET].view(U))
    one = jac(api, table, root, dof, 1, ids=[29])
    assert one.shape == (n, 1, 6, 39) and np.array_equal(one.view(U), J[:, [29]].view(U))
    # 640 m out: the same bits
    far = root.copy()
    far[:, 0:2] += np.array([640.0, -640.0], F)
    assert np.array_equal(jac(api, table, far, dof, 1).view(U), J.view(U))
    Mf, CJf = mm(api, table, far, dof, ms, arm, 1)
    assert np.array_equal(Mf.view(U), M.view(U)) and np.array_equal(CJf.view(U), CJ.view(U))
    # a NaN stays in its env, and the structural zeros are stored whatever the state holds
    bad_r, bad_d = root.copy(), dof.copy()
    bad_r[2, 4], bad_d[G + 1, 20, 0] = np.nan, np.inf
    Jn, (Mn, CJn) = jac(api, table, bad_r, bad_d, 1, finite=False), mm(api, table, bad_r, bad_d, ms, arm, 1, finite=False)
    keep = [e for e in range(n) if e not in (2, G + 1)]
    for a, b in ((Jn, J), (Mn, M), (CJn, CJ)):
        assert np.array_equal(a[keep].view(U), b[keep].view(U))
    assert np.isnan(Jn[2]).any() and np.isnan(Mn[2]).any() and np.isnan(CJn[2]).any() and np.isnan(Jn[G + 1, 27]).any() and np.isnan(Mn[G + 1]).any()
    mask = np.broadcast_to(JR.dof_mask()[:, None, :], (38, 6, 39))
    assert (Jn.view(U)[:, ~mask] == 0).all() and np.isfinite(Jn[:, 0]).all()
    # an id of 38 is refused, and nothing was launched
    assert jac(api, table, root, dof, 1, ids=[0, 38], expect=-1) is None and b"outside 0..37" in api["last_error"]()


def test_output_selection(api, table):
    """mass_matrix with and without the COM Jacobian, mass scale and armature: the same bits where the same is asked."""
    n = G + 3
    root, dof, ms = R.states(n, 10, mass=True)
    arm = JR.armature_of(n, 11)
    M, CJ = mm(api, table, root, dof, ms, arm, 0)
    M1, none = mm(api, table, root, dof, ms, arm, 0, cj=False)
    assert none is None and np.array_equal(M1.view(U), M.view(U))
    M2, CJ2 = mm(api, table, root, dof, ms, None, 0)
    j = np.arange(33)
    assert np.array_equal(CJ2.view(U), CJ.view(U))
    off = ~np.eye(39, dtype=bool)
    assert np.array_equal(M2[:, off].view(U), M[:, off].view(U)) and np.array_equal(M2[:, :6, :6].view(U), M[:, :6, :6].view(U))
    assert np.array_equal((M2[:, 6 + j, 6 + j] + arm).view(U), M[:, 6 + j, 6 + j].view(U))          # the armature is added last
    M3, CJ3 = mm(api, table, root, dof, None, None, 0)
    ex = JR.excess(root, dof, None, None, 0, None, M3, CJ3)
    assert JR.within(ex), ex


def test_unaligned_outputs_take_the_word_path(api, table):
    """Outputs 4 bytes past a 16-byte boundary: the same bits, written word by word, none outside."""
    n = G + 3
    root, dof, ms = R.states(n, 12, mass=True)
    J, (M, CJ) = jac(api, table, root, dof, 0), mm(api, table, root, dof, ms, None, 0)
    d = [dev(root), dev(dof), dev(ms)]
    bj, bm, bc = nan_buffer(n * 38 * 234, 1), nan_buffer(n * 1521, 1), nan_buffer(n * 117, 1)
    assert bj.data_ptr() % 16 == 0 and bm.data_ptr() % 16 == 0 and bc.data_ptr() % 16 == 0
    assert api["jacobian"](n, table.data_ptr(), ptr(d[0]), ptr(d[1]), None, 0, 0, bj.data_ptr() + 4, stream()) == 0
    assert api["mass_matrix"](n, table.data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), None, 0, bm.data_ptr() + 4, bc.data_ptr() + 4, stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(taken(bj, n * 38 * 234, 1).view(U), J.reshape(-1).view(U))
    assert np.array_equal(taken(bm, n * 1521, 1).view(U), M.reshape(-1).view(U))
    assert np.array_equal(taken(bc, n * 117, 1).view(U), CJ.reshape(-1).view(U))


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_jacobian_times_nu_is_what_dwb_refresh_reports(api, table, vel_at_com):
    """jacobian @ nu against the velocities and the COM velocity dwb_refresh itself returns on the same state, within the sum of both
    allowances: |nu|' (4 d_J) per row for the product, plus 4 d of body_states_ref for the tensor."""
    n = 3 * G + 5
    root, dof, ms = R.states(n, 13 + vel_at_com, mass=True)
    J = jac(api, table, root, dof, vel_at_com).astype(np.float64)
    _, CJ = mm(api, table, root, dof, ms, None, vel_at_com)
    bapi = B.declare(__import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0])
    btab = torch.from_numpy(B.pack_table(bapi, load_model()).view(np.int32)).to(DEV)
    d = [dev(root), dev(dof), dev(ms)]
    st, cm = torch.zeros(n, 38, 13, device=DEV), torch.zeros(n, 7, device=DEV)
    assert bapi["refresh"](n, btab.data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), None, 0, vel_at_com, st.data_ptr(), cm.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    st, cm = st.cpu().numpy().astype(np.float64), cm.cpu().numpy().astype(np.float64)
    nu = JR.nu(root, dof)
    dj, db = JR.measured(vel_at_com), R.measured(vel_at_com)
    s1 = np.abs(nu).sum(-1)[:, None, None]
    got = np.einsum("nkic,nc->nki", J, nu)
    el = np.abs(got[..., 0:3] - st[..., 7:10]) / (JR.FACTOR * dj["J_lin"] * s1 + R.FACTOR * db["vel"])
    ea = np.abs(got[..., 3:6] - st[..., 10:13]) / (JR.FACTOR * dj["J_ang"] * s1 + R.FACTOR * db["w"])
    ec = np.abs(np.einsum("nic,nc->ni", CJ.astype(np.float64), nu) - cm[:, 3:6]) / (JR.FACTOR * dj["com_jac"] * s1[:, 0] + R.FACTOR * db["com_vel"])
    print("J nu against dwb_refresh: linear %.3f, angular %.3f, COM %.3f of the allowance" % (el.max(), ea.max(), ec.max()))
    assert el.max() <= 1 and ea.max() <= 1 and ec.max() <= 1


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
        cfg["sim"]["mi355"]["jacobians"] = spec
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def actions(n, steps, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    amp = torch.tensor([0.0, 0.05, 0.3, 1.0], device=DEV)[torch.arange(n, device=DEV) % 4].view(1, n, 1)
    return ((torch.rand(steps, n, 13, generator=g, device=DEV) * 2 - 1) * amp).contiguous()


def bits(*ts):
    return torch.cat([t.reshape(-1).view(torch.int32) if t.dtype == torch.float32 else t.reshape(-1).to(torch.int32) for t in ts])


def test_live_env_with_resets(api, table):
    n, steps = 64, 40
    acts = actions(n, steps)
    runs = {}
    for name, spec, mi in (("off", None, {}), ("auto", {"com_jacobian": True, "auto": True}, {}),
                           ("subset", {"bodies": ["Head_Link", "L_Foot_Link", "R_Foot_Link"], "mass_matrix": False, "auto": True}, {"episode_stats": True})):
        env = make_env(n, spec, **mi)
        a, h, resets = torch.zeros(n, 13, device=DEV), [], 0
        if spec is None:
            assert env.jacobians is None
            with pytest.raises(RuntimeError, match="sim.mi355.jacobians"):
                env.refresh_jacobian_tensors()
            with pytest.raises(RuntimeError, match="sim.mi355.jacobians"):
                env.refresh_mass_matrix_tensors()
        for i in range(steps):
            a.copy_(acts[i])
            o, r, d, _ex = env.step(a)
            h.append(bits(o["obs"], r, d, env._buf["root_states"]))
            resets += int(d.sum())
            if name == "auto" and (i % 3 == 0 or i == steps - 1):
                jc = env.jacobians
                held = [t.cpu().numpy().copy() for t in (jc.jacobian, jc.mass_matrix, jc.com_jacobian)]
                b = env._buf
                root, dof, ms, arm = (b[k].cpu().numpy().reshape(s) for k, s in (("root_states", (n, 13)), ("dof_state", (n, 33, 2)),
                                                                                ("mass_scale", (n, 38)), ("dof_armature", (n, 33))))
                J = jac(api, table, root, dof, jc.vel_at_com)
                M, CJ = mm(api, table, root, dof, ms, arm, jc.vel_at_com)
                for got, want in zip(held, (J, M, CJ)):
                    assert np.array_equal(got.view(U), want.view(U)), i
                if i % 12 == 0 or i == steps - 1:
                    ex = JR.excess(root, dof, ms, arm, jc.vel_at_com, J, M, CJ)
                    assert JR.within(ex), (i, ex)
        if name == "auto":
            assert jc.vel_at_com == 1 and jc.names == load_model().body_names and jc.dof_names == load_model().dof_names
            assert jc.jacobian.shape == (n, 38, 6, 39) and jc.mass_matrix.shape == (n, 39, 39) and jc.com_jacobian.shape == (n, 3, 39)
            assert jc.mm.shape == (n, 33, 33) and jc.mm.data_ptr() == jc.mass_matrix.data_ptr() + 4 * (6 * 39 + 6)
            assert jc.dof_mask.shape == (38, 39) and jc.dof_mask.dtype == torch.bool
            assert bool((jc.jacobian[:, ~jc.dof_mask[:, None, :].expand(38, 6, 39)] == 0).all())
            assert jc.index("Head_Link") == 29 and torch.equal(jc.rows("R_Foot_Link", "Head_Link"), jc.jacobian[:, [16, 29]])
            assert env.refresh_jacobian_tensors() is jc.jacobian and env.refresh_mass_matrix_tensors() is jc.mass_matrix
            # reset_idx refreshes too: the tensors are those of the buffers after it
            before = jc.jacobian.clone()
            env.reset_idx(torch.arange(0, n, 2, device=DEV))
            held = jc.jacobian.clone()
            assert torch.equal(env.refresh_jacobian_tensors(), held) and not torch.equal(held[0::2], before[0::2]) and torch.equal(held[1::2], before[1::2])
        if name == "subset":
            jc = env.jacobians
            assert jc.mass_matrix is None and jc.mm is None and jc.com_jacobian is None and jc.names == ["Head_Link", "L_Foot_Link", "R_Foot_Link"]
            assert jc.ids == [29, 8, 16] and jc.jacobian.shape == (n, 3, 6, 39) and jc.dof_mask.shape == (3, 39)
            with pytest.raises(RuntimeError, match="mass_matrix"):
                env.refresh_mass_matrix_tensors()
        runs[name] = torch.stack(h).cpu()
        env.close()
        assert resets > 0          # (the time limit alone resets every env)
    # the feature only reads: the same bits with the key absent, on, and on beside another recorder in a rebuilt env
    assert torch.equal(runs["off"], runs["auto"]) and torch.equal(runs["off"], runs["subset"])


def test_captured_step_plus_refreshes_replays_the_eager_bits():
    """Step and both refreshes recorded in one graph on one stream (a linear chain), replayed 10 times, against 10 eager steps from the same
    state."""
    n = 64
    acts = actions(n, 11, seed=3)
    outs = []
    for captured in (False, True):
        env = make_env(n, {"com_jacobian": True, "auto": True})
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
            jc = env.jacobians
            h.append(bits(jc.jacobian, jc.mass_matrix, jc.com_jacobian, env._buf["root_states"]))
        torch.cuda.synchronize()
        outs.append(torch.stack(h).cpu())
        env.close()
    assert torch.equal(outs[0], outs[1])


def test_tocabi_amp_lower(api, table):
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    n = 32
    cfg = default_amp_cfg(n, DEV)
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert amp.jacobians is None
    with pytest.raises(RuntimeError, match="amp_jacobians"):
        amp.refresh_jacobian_tensors()
    with pytest.raises(RuntimeError, match="amp_jacobians"):
        amp.refresh_mass_matrix_tensors()
    amp.close()
    cfg = default_amp_cfg(n, DEV)
    cfg["sim"].setdefault("mi355", {})["amp_jacobians"] = {"com_jacobian": True}
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert isinstance(amp.jacobians, JM.Jacobians) and amp._phys.jacobians is None
    jc = amp.jacobians
    assert jc.vel_at_com == int(amp._phys._ccfg.root_vel_at_com)
    g = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(20):
        amp.step((torch.rand(n, amp.num_actions, generator=g, device=DEV) * 2 - 1) * 0.1)
    assert amp.refresh_jacobian_tensors() is jc.jacobian and amp.refresh_mass_matrix_tensors() is jc.mass_matrix
    b = amp._phys._buf
    root, dof, ms, arm = (b[k].cpu().numpy().reshape(s) for k, s in (("root_states", (n, 13)), ("dof_state", (n, 33, 2)), ("mass_scale", (n, 38)),
                                                                    ("dof_armature", (n, 33))))
    ex = JR.excess(root, dof, ms, arm, jc.vel_at_com, jc.jacobian.cpu().numpy(), jc.mass_matrix.cpu().numpy(), jc.com_jacobian.cpu().numpy(),
                   report="TocabiAMPLower")
    amp.close()
    assert JR.within(ex), ex


# ---------------------------------------------------------------------------------------------- the player
def test_player_writes_the_dynamics(tmp_path):
    import importlib.util
    import os
    import subprocess
    import sys
    from isaacgymdyros_amd import ppo_checkpoint as PK
    from isaacgymdyros_amd import ppo_update as UP
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ppo_consumer", os.path.join(root, "examples", "ppo_consumer.py"))
    ppo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ppo)
    torch.manual_seed(3)
    net = ppo.DyrosActorCritic(UP.IN, UP.ACT, ppo.TRAIN_CFG["network"]).to(DEV)          # an untrained policy
    c = ppo.TRAIN_CFG["config"]
    ck = PK.save(str(tmp_path / "p.pth"), net, epoch=0, opt_actor=torch.optim.Adam(net.actor_parameters(), lr=c["learning_rate"]),
                 opt_critic=torch.optim.Adam(net.critic_parameters(), lr=c["critic_lr"]))
    out = tmp_path / "dynamics"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "examples", "ppo_player.py"), "--checkpoint", ck, "--num-envs", "64",
                        "--games", "64", "--max-steps", "60", "--episode-length", "0.1", "--dynamics-dir", str(out), "--dynamics-envs", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["dynamics_env0.npz", "dynamics_env1.npz"]
    z = np.load(out / "dynamics_env1.npz")
    T = z["jacobian"].shape[0]
    assert 20 <= T <= 60 and z["jacobian"].shape == (T, 3, 6, 39) and z["mass_matrix"].shape == (T, 39, 39) and z["com_jacobian"].shape == (T, 3, 39)
    assert float(z["dt"]) == pytest.approx(0.004)
    assert z["names"].tolist() == ["Head_Link", "L_Foot_Link", "R_Foot_Link"] and z["dof_names"].tolist() == load_model().dof_names
    M = z["mass_matrix"]
    assert np.isfinite(z["jacobian"]).all() and np.isfinite(M).all() and np.array_equal(M, np.swapaxes(M, 1, 2))
    total = M[:, 0, 0]
    assert (total > 50).all() and np.array_equal(M[:, 1, 1], total) and (np.diagonal(M, axis1=1, axis2=2) > 0).all()
