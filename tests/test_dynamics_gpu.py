"""The bias-force, gravity, inverse-dynamics and momentum tensors on an MI355X (include/dyros_dynamics.h, csrc/dw_dynamics.hip, DESIGN.md
section 24): the HIP kernel against the float64 reference of tests/dynamics_ref.py under its measured tolerance at the workgroup's edges, with
the output buffers filled with NaN, too long, and their tails watched; the ways to choose outputs; unaligned outputs; agreement with the
shipped dwj_mass_matrix and dwb_refresh; the outputs' exact properties; a live env with resets; a captured step plus both calls;
TocabiAMPLower; the player's files."""
import numpy as np
import pytest
import torch

import body_states_ref as R
import dynamics_ref as DR
import jacobians_ref as JR
from isaacgymdyros_amd import body_states as B
from isaacgymdyros_amd import dynamics as DM
from isaacgymdyros_amd import jacobians as JM
from isaacgymdyros_amd.model import load_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = DM.GROUP          # envs per workgroup
PAD = 64
F, U = np.float32, np.uint32
OUTS = ("bias", "gravity", "tau", "momentum")
WORDS = {"bias": 39, "gravity": 39, "tau": 39, "momentum": 6}


def stream():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return __import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0]


@pytest.fixture(scope="module")
def api():
    return DM.declare(lib())


@pytest.fixture(scope="module")
def table(api):
    return torch.from_numpy(DM.pack_table(api, load_model()).view(np.int32)).to(DEV)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t, offset=0):
    return None if t is None else t.data_ptr() + 4 * offset


def run(api, table, root, dof, ms, arm, acc, vel_at_com, outs=OUTS, g=DR.GRAVITY, offset=0, finite=True, expect=0):
    """One launch into NaN-filled buffers PAD words too long (and `offset` words past their start); returns the outputs named as a dict (the
    others None): every word written (when the inputs were finite), none outside."""
    n = len(root)
    d = [dev(root), dev(dof), dev(ms), dev(arm), dev(acc)]
    buf = {k: torch.full((offset + n * WORDS[k] + PAD,), float("nan"), device=DEV) if k in outs else None for k in OUTS}
    assert all(b is None or b.data_ptr() % 16 == 0 for b in buf.values())
    rc = api["inverse_dynamics"](n, table.data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), g[0], g[1], g[2], ptr(d[4]), vel_at_com,
                                 ptr(buf["bias"], offset), ptr(buf["gravity"], offset), ptr(buf["tau"], offset), ptr(buf["momentum"], offset), stream())
    torch.cuda.synchronize()          # (d is freed after this)
    assert rc == expect, api["last_error"]()
    out = {}
    for k in OUTS:
        if buf[k] is None:
            out[k] = None
            continue
        h, words = buf[k].cpu().numpy(), n * WORDS[k]
        if rc != 0:
            assert np.isnan(h).all()          # nothing was launched
            out[k] = None
            continue
        assert np.isnan(h[:offset]).all() and np.isnan(h[offset + words:]).all(), "a word outside %s was written" % k
        o = h[offset:offset + words]
        if finite:
            assert np.isfinite(o).all(), "%d words of %s were not written" % (int(np.isnan(o).sum()), k)
        out[k] = o.reshape(n, WORDS[k]).copy()
    return out


def same(a, b):
    """Number for number: equal as floats (a zero's sign apart), NaN nowhere."""
    return bool(np.isfinite(a).all() and np.isfinite(b).all() and (a == b).all())


# ---------------------------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize("vel_at_com", [0, 1])
@pytest.mark.parametrize("n", [1, G - 1, G, G + 1, 3 * G + 5])
def test_kernel_against_float64(api, table, n, vel_at_com):
    """n = 1: one env in one workgroup; G - 1, G, G + 1: the group's edge; 3 G + 5: four whole groups and a partial one."""
    root, dof, ms, arm, acc = DR.seeded(n, 100 * n + vel_at_com)
    o = run(api, table, root, dof, ms, arm, acc, vel_at_com)
    ex = DR.excess(o, root, dof, ms, arm, acc, vel_at_com, report="gpu n=%d vel_at_com=%d" % (n, vel_at_com))
    assert len(ex) == len(DR.CHANNELS) and DR.within(ex), ex


def test_output_selection_and_unaligned_outputs(api, table):
    """Every single output, all four, with and without mass scale and armature, and every output 4 bytes past a 16-byte boundary: the same
    bits where the same is asked."""
    n = 2 * G + 3
    root, dof, ms, arm, acc = DR.seeded(n, 10)
    full = run(api, table, root, dof, ms, arm, acc, 0)
    for k in OUTS:
        one = run(api, table, root, dof, ms, arm, acc, 0, outs=(k,))
        assert np.array_equal(one[k].view(U), full[k].view(U)), k
        rest = run(api, table, root, dof, ms, arm, acc, 0, outs=tuple(j for j in OUTS if j != k))
        assert all(np.array_equal(rest[j].view(U), full[j].view(U)) for j in OUTS if j != k), k
    o = run(api, table, root, dof, ms, arm, None, 0, outs=("bias", "gravity", "momentum"))          # no accel
    assert all(np.array_equal(o[j].view(U), full[j].view(U)) for j in ("bias", "gravity", "momentum"))
    off = run(api, table, root, dof, ms, arm, acc, 0, offset=1)
    assert all(np.array_equal(off[k].view(U), full[k].view(U)) for k in OUTS)
    # the armature is added last, on the joints only, and enters tau alone
    na = run(api, table, root, dof, ms, None, acc, 0)
    assert np.array_equal(na["tau"][:, :6].view(U), full["tau"][:, :6].view(U)) and np.array_equal((na["tau"][:, 6:] + arm * acc[:, 6:]).view(U), full["tau"][:, 6:].view(U))
    assert all(np.array_equal(na[k].view(U), full[k].view(U)) for k in ("bias", "gravity", "momentum"))
    # nominal masses, no armature, another gravity vector, vel_at_com
    g = (1.5, -2.0, -3.71)
    nom = run(api, table, root, dof, None, None, acc, 1, g=g)
    ex = DR.excess(nom, root, dof, None, None, acc, 1, g=g, report="gpu, nominal masses, no armature, g = %s" % (g,))
    assert DR.within(ex), ex
    # refused before any launch: nothing is written
    assert run(api, table, root, dof, ms, arm, None, 0, outs=("tau",), expect=-1)["tau"] is None and b"tau needs accel" in api["last_error"]()
    assert run(api, table, root, dof, ms, arm, acc, 0, g=(0.0, float("nan"), -9.81), expect=-1)["bias"] is None and b"not finite" in api["last_error"]()


@pytest.mark.parametrize("vel_at_com", [0, 1])
def test_against_the_shipped_kernels(api, table, vel_at_com):
    """tau - bias against dwj_mass_matrix's own M times accel (the product in float64 on the host), within the sum of the two allowances:
    (4 d_M)' |accel| per row for the product, 4 d_tau + 4 d_bias for the difference.  momentum[:, 0:3] and gravity[:, 0:3] against dwb_refresh's
    com (COM velocity and mass): 4 d of each factor through the product."""
    n = 3 * G + 5
    root, dof, ms, arm, acc = DR.seeded(n, 13 + vel_at_com)
    o = run(api, table, root, dof, ms, arm, acc, vel_at_com)
    d = [dev(root), dev(dof), dev(ms), dev(arm)]
    japi = JM.declare(lib())
    M = torch.zeros(n, 39, 39, device=DEV)
    assert japi["mass_matrix"](n, table.data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), vel_at_com, M.data_ptr(), None, stream()) == 0
    bapi = B.declare(lib())
    btab = torch.from_numpy(B.pack_table(bapi, load_model()).view(np.int32)).to(DEV)
    st, cm = torch.zeros(n, 38, 13, device=DEV), torch.zeros(n, 7, device=DEV)
    assert bapi["refresh"](n, btab.data_ptr(), ptr(d[0]), ptr(d[1]), ptr(d[2]), None, 0, vel_at_com, st.data_ptr(), cm.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    M, cm, a = M.cpu().numpy().astype(np.float64), cm.cpu().numpy().astype(np.float64), acc.astype(np.float64)
    dn, db = DR.measured(vel_at_com), R.measured(vel_at_com)
    row = np.array([dn["tau_lin"] + dn["bias_lin"]] * 3 + [dn["tau_ang"] + dn["bias_ang"]] * 3 + [dn["tau_joint"] + dn["bias_joint"]] * 33)
    allow = np.abs(a) @ JR.allowance(vel_at_com).T + DR.FACTOR * row
    err = np.abs(o["tau"].astype(np.float64) - o["bias"].astype(np.float64) - np.einsum("nab,nb->na", M, a))
    e1 = (err / allow).max()
    mass, cv = cm[:, 6:7], cm[:, 3:6]
    e2 = (np.abs(o["momentum"][:, 0:3] - mass * cv) / (DR.FACTOR * dn["momentum_lin"] + R.FACTOR * (db["mass"] * np.abs(cv) + mass * db["com_vel"]))).max()
    g = np.asarray(DR.GRAVITY, F).astype(np.float64)
    e3 = (np.abs(o["gravity"][:, 0:3] + mass * g) / (DR.FACTOR * dn["gravity_lin"] + R.FACTOR * db["mass"] * np.abs(g) + 1e-30)).max()
    print("tau - bias against dwj M a: %.3f; momentum against dwb com: %.3f; gravity against dwb mass: %.3f of the allowance" % (e1, e2, e3))
    assert e1 <= 1 and e2 <= 1 and e3 <= 1


def test_exact_properties(api, table):
    n = 2 * G + 3
    root, dof, ms, arm, acc = DR.seeded(n, 8)
    o = run(api, table, root, dof, ms, arm, acc, 1)
    # 640 m out: the same bits
    far = root.copy()
    far[:, 0:2] += np.array([640.0, -640.0], F)
    of = run(api, table, far, dof, ms, arm, acc, 1)
    assert all(np.array_equal(of[k].view(U), o[k].view(U)) for k in OUTS)
    # every velocity zeroed: bias is gravity, the momentum is zero
    still_r, still_d = root.copy(), dof.copy()
    still_r[:, 7:13], still_d[:, :, 1] = 0, 0
    os_ = run(api, table, still_r, still_d, ms, arm, acc, 1)
    assert same(os_["bias"], os_["gravity"]) and same(os_["gravity"], o["gravity"]) and (os_["momentum"] == 0).all()
    # accel = 0: tau is bias
    oz = run(api, table, root, dof, ms, arm, np.zeros_like(acc), 1)
    assert same(oz["tau"], oz["bias"]) and np.array_equal(oz["bias"].view(U), o["bias"].view(U))
    # a NaN stays in its env; one in accel reaches tau alone
    bad_r, bad_d, bad_a = root.copy(), dof.copy(), acc.copy()
    bad_r[2, 4], bad_d[G + 1, 20, 0], bad_a[7, 7] = np.nan, np.inf, np.nan
    on = run(api, table, bad_r, bad_d, ms, arm, bad_a, 1, finite=False)
    keep = [e for e in range(n) if e not in (2, G + 1, 7)]
    for k in OUTS:
        assert np.array_equal(on[k][keep].view(U), o[k][keep].view(U)), k
        assert np.isnan(on[k][2]).any() and np.isnan(on[k][G + 1]).any(), k
    assert np.isnan(on["tau"][7]).any() and all(np.array_equal(on[k][7].view(U), o[k][7].view(U)) for k in ("bias", "gravity", "momentum"))


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
        cfg["sim"]["mi355"]["dynamics"] = spec
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def actions(n, steps, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    amp = torch.tensor([0.0, 0.05, 0.3, 1.0], device=DEV)[torch.arange(n, device=DEV) % 4].view(1, n, 1)
    return ((torch.rand(steps, n, 13, generator=g, device=DEV) * 2 - 1) * amp).contiguous()


def bits(*ts):
    return torch.cat([t.contiguous().reshape(-1).view(torch.uint8) for t in ts])


def buffers(env, n):
    b = env._buf
    return tuple(b[k].cpu().numpy().reshape(s) for k, s in (("root_states", (n, 13)), ("dof_state", (n, 33, 2)), ("mass_scale", (n, 38)), ("dof_armature", (n, 33))))


def test_live_env_with_resets(api, table):
    n, steps = 64, 40
    acts = actions(n, steps)
    runs = {}
    every = {"inverse_dynamics": True, "momentum": True, "auto": True}
    for name, spec, mi in (("off", None, {}), ("auto", every, {}), ("beside", {"bias": False, "auto": True}, {"episode_stats": True})):
        env = make_env(n, spec, **mi)
        a, h, resets = torch.zeros(n, 13, device=DEV), [], 0
        if spec is None:
            assert env.dynamics is None
        for i in range(steps):
            a.copy_(acts[i])
            o, r, d, _ex = env.step(a)
            h.append(bits(o["obs"], r, d, env._buf["root_states"], env._buf["env_state"]))
            resets += int(d.sum())
            if name == "auto" and (i % 3 == 0 or i == steps - 1):
                dy = env.dynamics
                held = {k: getattr(dy, k).cpu().numpy().copy() for k in ("bias", "gravity", "momentum")}
                root, dof, ms, arm = buffers(env, n)
                acc = DR.accel_of(n, i)
                tau = dy.inverse_dynamics(torch.from_numpy(acc).to(DEV)).cpu().numpy()
                fresh = run(api, table, root, dof, ms, arm, acc, dy.vel_at_com, g=dy.g)
                assert all(np.array_equal(held[k].view(U), fresh[k].view(U)) for k in held) and np.array_equal(tau.view(U), fresh["tau"].view(U)), i
                if i % 12 == 0 or i == steps - 1:
                    ex = DR.excess(fresh, root, dof, ms, arm, acc, dy.vel_at_com, g=dy.g)
                    assert DR.within(ex), (i, ex)
        if name == "auto":
            assert dy.vel_at_com == 1 and dy.g == (0.0, 0.0, -9.81) and dy.dof_names == load_model().dof_names
            assert dy.bias.shape == dy.gravity.shape == dy.tau.shape == dy.accel.shape == (n, 39) and dy.momentum.shape == (n, 6)
            assert dy.joint_gravity.shape == (n, 33) and dy.joint_gravity.data_ptr() == dy.gravity.data_ptr() + 24
            # reset_idx refreshes too: the tensors are those of the buffers after it
            before = dy.gravity.clone()
            env.reset_idx(torch.arange(0, n, 2, device=DEV))
            held = dy.gravity.clone()
            dy.refresh()
            assert torch.equal(dy.gravity, held) and not torch.equal(held[0::2], before[0::2]) and torch.equal(held[1::2], before[1::2])
        if name == "beside":
            dy = env.dynamics
            assert dy.bias is None and dy.tau is None and dy.accel is None and dy.momentum is None and dy.gravity.shape == (n, 39)
            with pytest.raises(RuntimeError, match="inverse_dynamics"):
                dy.inverse_dynamics()
            root, dof, ms, arm = buffers(env, n)
            fresh = run(api, table, root, dof, ms, arm, None, dy.vel_at_com, outs=("gravity",))
            assert np.array_equal(dy.gravity.cpu().numpy().view(U), fresh["gravity"].view(U))
        runs[name] = torch.stack(h).cpu()
        env.close()
        assert resets > 0          # (the time limit alone resets every env)
    # the feature only reads: the same bits with the key absent, on, and on beside another recorder in a rebuilt env
    assert torch.equal(runs["off"], runs["auto"]) and torch.equal(runs["off"], runs["beside"])


def test_captured_step_plus_both_calls_replays_the_eager_bits():
    """Step, refresh() (auto) and inverse_dynamics() recorded in one graph on one stream (a linear chain), replayed 10 times, against 10 eager
    steps from the same state."""
    n = 64
    acts = actions(n, 11, seed=3)
    accs = torch.from_numpy(np.stack([DR.accel_of(n, 50 + i) for i in range(11)])).to(DEV)
    outs = []
    for captured in (False, True):
        env = make_env(n, {"inverse_dynamics": True, "momentum": True, "auto": True})
        dy = env.dynamics
        a = torch.zeros(n, 13, device=DEV)
        a.copy_(acts[0])
        env.step(a)                            # (the first step is eager on both sides)
        dy.inverse_dynamics(accs[0])
        torch.cuda.synchronize()
        h = []
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            a.copy_(acts[1])
            with torch.cuda.graph(g, stream=side):
                env.step(a)
                dy.inverse_dynamics()
            # (the capture itself ran nothing: replay the recorded step for each of the 10 actions)
        for i in range(1, 11):
            a.copy_(acts[i])
            dy.accel.copy_(accs[i])
            if captured:
                g.replay()
            else:
                env.step(a)
                dy.inverse_dynamics()
            h.append(bits(dy.bias, dy.gravity, dy.tau, dy.momentum, env._buf["root_states"]))
        torch.cuda.synchronize()
        outs.append(torch.stack(h).cpu())
        env.close()
    assert torch.equal(outs[0], outs[1])


def test_tocabi_amp_lower():
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    n = 32
    cfg = default_amp_cfg(n, DEV)
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert amp.dynamics is None
    amp.close()
    cfg = default_amp_cfg(n, DEV)
    cfg["sim"].setdefault("mi355", {})["amp_dynamics"] = {"inverse_dynamics": True, "momentum": True, "auto": True}
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert isinstance(amp.dynamics, DM.Dynamics) and amp._phys.dynamics is None
    dy = amp.dynamics
    assert dy.vel_at_com == int(amp._phys._ccfg.root_vel_at_com)
    g = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(20):
        amp.step((torch.rand(n, amp.num_actions, generator=g, device=DEV) * 2 - 1) * 0.1)
    acc = DR.accel_of(n, 7)
    tau = dy.inverse_dynamics(torch.from_numpy(acc).to(DEV))
    assert tau is dy.tau
    root, dof, ms, arm = buffers(amp._phys, n)
    got = {k: getattr(dy, k).cpu().numpy() for k in OUTS}          # (bias, gravity, momentum: what the last step's auto refresh left)
    ex = DR.excess(got, root, dof, ms, arm, acc, dy.vel_at_com, g=dy.g, report="TocabiAMPLower")
    amp.close()
    assert len(ex) == len(DR.CHANNELS) and DR.within(ex), ex


# ---------------------------------------------------------------------------------------------- the player
def test_player_writes_the_forces(tmp_path):
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
    files = {}
    for name, flag in (("plain", []), ("forces", ["--dynamics-forces"])):
        out = tmp_path / name
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "examples", "ppo_player.py"), "--checkpoint", ck, "--num-envs", "64",
                            "--games", "64", "--max-steps", "60", "--episode-length", "0.1", "--dynamics-dir", str(out), "--dynamics-envs", "2"] + flag,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["dynamics_env0.npz", "dynamics_env1.npz"]
        files[name] = np.load(out / "dynamics_env1.npz")
    plain, z = files["plain"], files["forces"]
    old = ["names", "dof_names", "dt", "jacobian", "mass_matrix", "com_jacobian"]
    assert sorted(plain.files) == sorted(old) and sorted(z.files) == sorted(old + ["bias", "gravity", "momentum"])
    assert all(np.array_equal(plain[k], z[k]) for k in old)          # (the same seed: the files are what they were, plus three arrays)
    T = z["jacobian"].shape[0]
    assert 20 <= T <= 60 and z["bias"].shape == (T, 39) and z["gravity"].shape == (T, 39) and z["momentum"].shape == (T, 6)
    assert all(np.isfinite(z[k]).all() for k in ("bias", "gravity", "momentum"))
    # the weight: gravity's force is -g times the total mass the mass matrix holds, to the two tensors' allowances
    total = z["mass_matrix"][:, 0, 0].astype(np.float64)
    d, dj = DR.measured(1), JR.measured(1)
    assert (z["gravity"][:, 0:2] == 0).all() and (np.abs(z["gravity"][:, 2] - 9.81 * total) <= DR.FACTOR * d["gravity_lin"] + 9.81 * JR.FACTOR * dj["M_bb"]).all()
