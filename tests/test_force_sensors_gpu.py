"""The foot force-torque sensors on an MI355X (include/dyros_sensors.h, csrc/dw_sensors.hip): the HIP kernel against
the float64 restatement of tests/force_sensors_ref.py under its measured tolerance at the workgroup's edges, with the output buffers too
long and their tails watched; the ways to choose outputs; the corners against BodyStates; a standing env against the step's own foot rows; a
live env with resets; a captured step plus refresh; TocabiAMPLower."""
import ctypes as C

import numpy as np
import pytest
import torch

import body_states_ref as BR
import force_sensors_ref as R
from isaacgymdyros_amd import body_states as B
from isaacgymdyros_amd import force_sensors as FS
from isaacgymdyros_amd.model import load_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = FS.GROUP          # envs per workgroup
PAD, SENTINEL = 64, -7.25
WORDS = {"cop": 8, "zmp": 4, "corners": 48}
SHAPES = {"cop": (2, 4), "zmp": (4,), "corners": (8, 6)}
ALL = ("sensors", "cop", "zmp", "corners")
F = np.float32


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def api():
    return FS.declare(__import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0])


@pytest.fixture(scope="module")
def table():
    lib = __import__("isaacgymdyros_amd._lib", fromlist=["load"]).load()[0]
    return torch.from_numpy(B.pack_table(B.declare(lib), load_model()).view(np.int32)).to(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).to(DEV)


def c_sensors(sensors):
    return FS.sensor_array([dict(s, pos=s.get("pos", [0, 0, -0.09]), quat=s.get("quat", [0, 0, 0, 1]), world_frame=s.get("world_frame", False))
                            for s in sensors])


def refresh(api, table, root, dof, es, sensors=R.DEFAULT_SENSORS, want=ALL, expect=0, arr=None, ns=None, shift=0):
    """dwf_refresh on numpy inputs (es: [n, 372] task records); every output is PAD words too long and filled with SENTINEL, and every word
    past the end (and, with shift, the `shift` words before the start) must come back untouched.  Returns a dict of numpy arrays (None where
    not asked for); after a refusal, the raw buffers."""
    n = len(root)
    ns = len(sensors) if ns is None else ns
    d = [dev(root), dev(dof), dev(es)]
    words = dict(WORDS, sensors=6 * min(ns, 8))
    bufs = {k: torch.full((shift + n * words[k] + PAD,), SENTINEL, device=DEV) if k in want and words[k] else None for k in ALL}
    ptr = lambda k: None if bufs[k] is None else bufs[k].data_ptr() + 4 * shift          # noqa: E731
    m = FS.model_struct(load_model(), R.DT)
    arr = (c_sensors(sensors) if len(sensors) else None) if arr is None else arr
    rc = api["refresh"](n, table.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), C.byref(m), arr if bufs["sensors"] is not None else None,
                        ns if bufs["sensors"] is not None else 0, ptr("sensors"), ptr("cop"), ptr("zmp"), ptr("corners"), stream())
    torch.cuda.synchronize()          # (d is freed after this)
    assert rc == expect, api["last_error"]()
    out = {}
    for k in ALL:
        if bufs[k] is None:
            out[k] = None
            continue
        h = bufs[k].cpu().numpy()
        nw = n * words[k]
        assert (h[:shift] == F(SENTINEL)).all() and (h[shift + nw:] == F(SENTINEL)).all(), (k, np.argwhere(h[shift + nw:] != F(SENTINEL))[:5])
        out[k] = h[shift:shift + nw].reshape((n,) + ((ns, 6) if k == "sensors" else SHAPES[k])) if rc == 0 else h
    return out


def records(warm, seed=1):
    return R.env_state_of(warm, fill=np.random.default_rng(seed))          # (random words around the impulse block: a read beside it shows)


# ---------------------------------------------------------------------------------------------- the kernel against float64
@pytest.mark.parametrize("n", [1, G - 1, G, G + 1, 3 * G + 5])
def test_kernel_against_float64(api, table, n):
    """n = 1: one env in one workgroup; G - 1, G, G + 1: the group's edge; 3 G + 5 = 53: three whole groups and a partial one.  The default two
    sensors and eight with repeats, mixed world_frame and non-identity quaternions; all four outputs."""
    root, dof, warm = R.states(n, 100 * n)
    for name, S in (("default", R.DEFAULT_SENSORS), ("eight", R.sensors8())):
        got = refresh(api, table, root, dof, records(warm), S)
        ex = R.excess(got, root, dof, warm, R.INV_DT, S, report="gpu n=%d %s" % (n, name))
        assert R.within(ex) and len(ex) == 10, ex


def test_kernel_640_m_out(api, table):
    n = 3 * G + 5
    root, dof, warm = R.states(n, 7, xy=640.0)
    got = refresh(api, table, root, dof, records(warm), R.sensors8())
    ex = R.excess(got, root, dof, warm, R.INV_DT, R.sensors8(), report="gpu 640 m")
    assert R.within(ex), ex
    assert np.abs(got["zmp"][:, 0:2]).max() > 600


def test_output_selection(api, table):
    n = 3 * G + 5
    root, dof, warm = R.states(n, 8)
    es, S = records(warm), R.sensors8()
    full = refresh(api, table, root, dof, es, S)
    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))          # noqa: E731
    one = refresh(api, table, root, dof, es, S[4:5], want=("sensors",))
    assert one["sensors"].shape == (n, 1, 6) and same(one["sensors"], full["sensors"][:, 4:5]) and one["cop"] is None
    two = refresh(api, table, root, dof, es, want=("sensors", "cop"))
    assert R.within(R.excess(two, root, dof, warm)) and same(two["cop"], full["cop"]) and two["zmp"] is None and two["corners"] is None
    for k in ("cop", "zmp", "corners"):
        part = refresh(api, table, root, dof, es, [], want=(k,))
        assert [x for x in ALL if part[x] is not None] == [k] and same(part[k], full[k]), k
        assert R.within(R.excess(part, root, dof, warm, sensors=[]))
    # a foot of 2 and nine sensors are refused, and nothing was launched: every buffer still holds the sentinel
    bad = c_sensors(S)
    bad[3].foot = 2
    for kw, msg in ((dict(arr=bad), b"foot is outside 0..1"), (dict(arr=(FS.DwfSensor * 9)(), ns=9), b"ns must be in 0..8")):
        raw = refresh(api, table, root, dof, es, S, expect=-1, **kw)
        assert msg in api["last_error"]() and all((v == F(SENTINEL)).all() for v in raw.values())


def test_unaligned_output_pointers_take_the_word_path(api, table):
    """Every output 4 bytes past a 16-byte boundary: the same bits, written word by word, the word before the start untouched."""
    n = G + 3
    root, dof, warm = R.states(n, 9)
    es, S = records(warm), R.sensors8()[:3]
    full = refresh(api, table, root, dof, es, S)
    off = refresh(api, table, root, dof, es, S, shift=1)
    for k in ALL:
        assert np.array_equal(off[k].view(np.uint32), full[k].view(np.uint32)), k


# ---------------------------------------------------------------------------------------------- envs
def make_env(n, spec=None, **mi):
    from isaacgymdyros_amd.config import default_cfg
    from isaacgymdyros_amd.dyros_dynamic_walk import DyrosDynamicWalk
    cfg = default_cfg(n, DEV)
    cfg["seed"] = 42
    cfg["env"]["episodeLength"] = 0.1          # (seconds; 0.004 s per policy step: every env meets the time limit at step 25)
    cfg["sim"]["mi355"]["device_step_counter"] = True
    cfg["sim"]["mi355"]["alias_obs"] = True
    cfg["env"].update(mi.pop("env", {}))
    cfg["sim"]["mi355"].update(mi)
    if spec is not None:
        cfg["sim"]["mi355"]["force_sensors"] = spec
    return DyrosDynamicWalk(cfg, DEV, 0, True)


def actions(n, steps, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    amp = torch.tensor([0.0, 0.05, 0.3, 1.0], device=DEV)[torch.arange(n, device=DEV) % 4].view(1, n, 1)
    return ((torch.rand(steps, n, 13, generator=g, device=DEV) * 2 - 1) * amp).contiguous()


def held(fs):
    return {"sensors": fs.sensors.cpu().numpy(), "cop": None if fs.cop is None else fs.cop.cpu().numpy(), "zmp": None if fs.zmp is None else fs.zmp.cpu().numpy(),
            "corners": None if fs.corners is None else fs.corners.cpu().numpy()}


def inputs(host):
    b = host._buf
    root, dof, es = (b[k].cpu().numpy() for k in ("root_states", "dof_state", "env_state"))
    return root, dof.reshape(len(root), 33, 2), es


def test_corners_against_body_states():
    """corners[:, :, 0:3] = the BodyStates rows of the two foot links + R(q) foot_pos (formed here in float64), within section 21's position
    allowance."""
    n = 64
    env = make_env(n, {"corners": True}, body_states={"bodies": ["L_Foot_Link", "R_Foot_Link"], "com": False})
    root, dof, _ = R.states(n, 10)
    env._buf["root_states"].copy_(torch.from_numpy(root))
    env._buf["dof_state"].copy_(torch.from_numpy(dof))
    st = env.refresh_rigid_body_state_tensor().cpu().numpy().astype(np.float64)
    env.refresh_force_sensor_tensor()
    cor = env.force_sensors.corners.cpu().numpy().astype(np.float64)
    env.close()
    want = np.stack([st[:, k // 4, 0:3] + BR.mv3(BR.qmat(st[:, k // 4, 3:7]), R.FOOT_POS[k][None, :]) for k in range(8)], 1)
    allow = BR.FACTOR * BR.measured(1)["off"] + BR.ulp(want)
    print("corners against BodyStates: %.2e m, %.2f of the allowance" % (np.abs(cor[..., 0:3] - want).max(), (np.abs(cor[..., 0:3] - want) / allow).max()))
    assert (np.abs(cor[..., 0:3] - want) <= allow).all()


def test_standing_env_against_the_steps_foot_rows():
    """N = 17, zero actions, 5 steps from reset, self-collision and pushes off: nothing but the soles touches, so the world-frame sensor forces
    are the feet's rows of contact_forces, within force_sensors_ref.step_force_tolerance (4 ulp of sum_k |f_k|, from the float32 format; the CPU
    oracle uses 0.36 of it)."""
    n = 17
    spec = {"sensors": [{"body": "L_Foot_Link", "world_frame": True}, {"body": "R_Foot_Link", "world_frame": True}], "corners": True}
    env = make_env(n, spec, self_collision=False, env={"perturbation": False})
    env.reset()
    a = torch.zeros(n, 13, device=DEV)
    for _ in range(5):
        _o, _r, d, _x = env.step(a)
        assert not d.any()
    env.refresh_force_sensor_tensor()
    fs = env.force_sensors
    lf, rf = env.model.left_foot_idx, env.model.right_foot_idx
    cf = env._buf["contact_forces"].cpu().numpy().astype(np.float64)
    got = fs.force.cpu().numpy().astype(np.float64)
    root, dof, es = inputs(env)
    warm = es[:, FS.K["DWF_ES_WARM"]:FS.K["DWF_ES_WARM"] + 24]
    loaded = fs.cop[..., 2].cpu().numpy()
    env.close()
    others = [g for g in range(38) if g not in (lf, rf)]
    assert not cf[:, others].any()
    err, allow = np.abs(got - cf[:, [lf, rf]]), R.step_force_tolerance(warm)
    print("standing env: Fz %s N, %.2f of the allowance used" % (loaded[0], (err / np.maximum(allow, 1e-30))[allow > 0].max()))
    assert (err <= allow).all(), (err.max(), allow.min())
    assert (loaded.max(1) > 0).all()          # at least one sole is loaded in every env


def bits(*ts):
    return torch.cat([t.reshape(-1).view(torch.int32) if t.dtype == torch.float32 else t.reshape(-1).to(torch.int32) for t in ts])


def test_live_env_with_resets(api, table):
    n, steps = 64, 40
    acts = actions(n, steps)
    runs, zero_rows = {}, 0
    for name, spec in (("off", None), ("auto", {"corners": True, "auto": True})):
        env = make_env(n, spec)
        a, h, resets = torch.zeros(n, 13, device=DEV), [], 0
        if spec is None:
            assert env.force_sensors is None
            with pytest.raises(RuntimeError):
                env.refresh_force_sensor_tensor()
        for i in range(steps):
            a.copy_(acts[i])
            o, r, d, _ex = env.step(a)
            h.append(bits(o["obs"], r, d, env._buf["root_states"], env._buf["env_state"]))
            resets += int(d.sum())
            if name == "auto":
                fs = env.force_sensors
                was = held(fs)
                root, dof, es = inputs(env)
                fresh = refresh(api, table, root, dof, es, [dict(s) for s in fs.specs])
                for k in ALL:
                    assert np.array_equal(was[k].view(np.uint32), fresh[k].view(np.uint32)), (i, k)
                gone = d.cpu().numpy().astype(bool)
                if gone.any():          # an env that reset in this step reads all-zero rows (its corners keep their positions)
                    zero_rows += int(gone.sum())
                    assert not was["sensors"][gone].any() and not was["cop"][gone].any() and not was["zmp"][gone].any() and not was["corners"][gone][..., 3:6].any()
                if i in (10, 20, steps - 1):          # (steps at which no env has just reset: the soles are loaded)
                    warm = es[:, FS.K["DWF_ES_WARM"]:FS.K["DWF_ES_WARM"] + 24]
                    assert np.abs(warm).max() > 0
                    ex = R.excess(was, root, dof, warm, R.INV_DT, fs.specs, report="live step %d" % i)
                    assert R.within(ex), (i, ex)
        if name == "auto":
            assert fs.names == ["L_Foot_Link", "R_Foot_Link"] and fs.index("R_Foot_Link") == 1 and fs.dt == pytest.approx(0.004)
            assert fs.force.shape == (n, 2, 3) and fs.torque.shape == (n, 2, 3) and fs.cop.shape == (n, 2, 4) and fs.zmp.shape == (n, 4) and fs.corners.shape == (n, 8, 6)
            v = env.refresh_force_sensor_tensor()
            assert v.shape == (n, 12) and v.data_ptr() == fs.sensors.data_ptr()
            # reset_idx refreshes too: the reset envs read zero, their corners sit at the reset pose's height
            ids = torch.arange(0, n, 2, device=DEV)
            env.reset_idx(ids)
            assert not fs.sensors[ids].any() and not fs.zmp[ids].any() and fs.sensors[1::2].any()
            assert not fs.corners[ids][..., 3:6].any() and float((fs.corners[ids][..., 2] - fs.corners[ids][..., 2].mean()).abs().max()) < 0.1
        runs[name] = torch.stack(h).cpu()
        env.close()
        assert resets >= n
    assert zero_rows >= n
    # the feature only reads: the same bits with the key absent and on
    assert torch.equal(runs["off"], runs["auto"])


def test_captured_step_plus_refresh_replays_the_eager_bits():
    """Step and refresh recorded in one graph on one stream (a linear chain), replayed 10 times, against 10 eager steps from the same state."""
    n = 64
    acts = actions(n, 11, seed=3)
    outs = []
    for captured in (False, True):
        env = make_env(n, {"corners": True, "auto": True})
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
            fs = env.force_sensors
            h.append(bits(fs.sensors, fs.cop, fs.zmp, fs.corners, env._buf["root_states"]))
        torch.cuda.synchronize()
        outs.append(torch.stack(h).cpu())
        env.close()
    assert torch.equal(outs[0], outs[1]) and outs[0][-1, :n * 12].any()


def test_tocabi_amp_lower_rows(api, table):
    """TocabiAMPLower with amp_force_sensors: rows = the reference applied to the physics host's buffers.  Its reset paths write the root and
    joint rows and leave the task record alone: after reset_done() the impulse block of a reset env is the bits it held
    before, so its rows are the last substep's forces at the reset pose's lever arms until the next step replaces them."""
    from isaacgymdyros_amd.tocabi_amp_lower import TocabiAMPLower, default_amp_cfg
    n = 64
    cfg = default_amp_cfg(n, DEV)
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    assert amp.force_sensors is None
    with pytest.raises(RuntimeError):
        amp.refresh_force_sensor_tensor()
    amp.close()
    cfg = default_amp_cfg(n, DEV)
    cfg["sim"].setdefault("mi355", {})["amp_force_sensors"] = {"corners": True, "auto": True}
    amp = TocabiAMPLower(cfg, DEV, 0, True)
    fs = amp.force_sensors
    assert isinstance(fs, FS.ForceSensors) and amp._phys.force_sensors is None
    inv_dt = F(1.0) / F(amp._phys.dt)
    assert fs._model_c.inv_dt == float(inv_dt)
    g = torch.Generator(device=DEV).manual_seed(1)
    W0 = FS.K["DWF_ES_WARM"]
    for i in range(12):
        amp.step((torch.rand(n, amp.num_actions, generator=g, device=DEV) * 2 - 1) * 0.1)
        if i in (3, 11):
            root, dof, es = inputs(amp._phys)
            warm = es[:, W0:W0 + 24]
            ex = R.excess(held(fs), root, dof, warm, inv_dt, fs.specs, report="amp step %d" % i)
            assert R.within(ex), (i, ex)
    assert np.abs(warm).max() > 0 and (fs.cop[..., 2].max(1).values > 0).any()
    before = amp._phys._buf["env_state"][:, W0:W0 + 24].clone()
    amp.reset_buf[::2] = 1
    _obs, ids = amp.reset_done()
    assert len(ids) >= n // 2
    assert torch.equal(amp._phys._buf["env_state"][:, W0:W0 + 24].view(torch.int32), before.view(torch.int32))          # the reset left the block alone
    amp.refresh_force_sensor_tensor()
    root, dof, es = inputs(amp._phys)
    ex = R.excess(held(fs), root, dof, es[:, W0:W0 + 24], inv_dt, fs.specs, report="amp after reset_done")
    amp.close()
    assert R.within(ex), ex


# ---------------------------------------------------------------------------------------------- the player
def test_player_writes_the_sensor_trajectories(tmp_path):
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
    out = tmp_path / "sensors"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(root, "examples", "ppo_player.py"), "--checkpoint", ck, "--num-envs", "64",
                        "--games", "64", "--max-steps", "60", "--episode-length", "0.1", "--sensors-dir", str(out), "--sensors-envs", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["sensors_env0.npz", "sensors_env1.npz"]
    z = np.load(out / "sensors_env1.npz")
    T = z["sensors"].shape[0]
    assert 20 <= T <= 60 and z["sensors"].shape == (T, 2, 6) and z["cop"].shape == (T, 2, 4) and z["zmp"].shape == (T, 4) and float(z["dt"]) == pytest.approx(0.004)
    assert z["names"].tolist() == ["L_Foot_Link", "R_Foot_Link"] and np.isfinite(z["sensors"]).all()
    # the soles carry the robot at some step, and the CoP stays inside the sole
    c8 = R.FOOT_POS.reshape(2, 4, 3)
    assert z["zmp"][:, 2].max() > 500 and (z["cop"][..., 0] >= c8[..., 0].min() - 1e-6).all() and (z["cop"][..., 0] <= c8[..., 0].max() + 1e-6).all()
